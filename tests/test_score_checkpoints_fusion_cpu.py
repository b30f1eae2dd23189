"""CPU: the command line of score_checkpoints --fusion (what it asks for and refuses, each with its message), the rule that ties
a held entry to its partner checkpoint, and the unchanged single-stream parse."""
import pytest

BASE = ['x.yaml', '--gt', 'gt.json', '--known', 'known.txt']
PARTNER = ['--fusion', '--partner_checkpoint', 'flow/checkpoint-16.ckpt', '--partner_data', 'flow_npy']


def _exit_message(argv):
    from opental_amd.common.score_checkpoints import parse_own
    with pytest.raises(SystemExit) as e:
        parse_own(argv)
    return str(e.value)


def test_partner_options_belong_to_fusion():
    for option in ('--partner_checkpoint', '--partner_data', '--partner_train_data'):
        message = _exit_message(BASE + [option, 'somewhere'])
        assert option in message and '--fusion' in message
    message = _exit_message(BASE + PARTNER[1:])
    assert '--partner_checkpoint, --partner_data' in message and 'add --fusion' in message


def test_fusion_names_the_partner_option_it_misses():
    assert '--partner_checkpoint' in _exit_message(BASE + ['--fusion'])
    assert '--partner_checkpoint' in _exit_message(BASE + ['--fusion', '--partner_data', 'flow_npy'])
    message = _exit_message(BASE + ['--fusion', '--partner_checkpoint', 'p.ckpt'])
    assert '--partner_data' in message and 'no default' in message and '--partner_checkpoint' not in message
    train = ['--open_set', '--open_metrics', '--threshold_from_train']
    message = _exit_message(BASE + PARTNER + train)
    assert '--partner_train_data' in message and 'no default' in message


def test_fusion_parse_keeps_the_flag_for_the_config_and_hands_out_the_partner():
    from opental_amd.common.score_checkpoints import parse_own
    own, rest = parse_own(BASE + PARTNER)
    assert rest == ['x.yaml', '--fusion']
    assert own['--partner_checkpoint'] == 'flow/checkpoint-16.ckpt' and own['--partner_data'] == 'flow_npy'
    assert own['--partner_train_data'] is None
    own, rest = parse_own(BASE + PARTNER + ['--open_set', '--open_metrics', '--threshold_from_train', '--partner_train_data', 'tr'])
    assert own['--partner_train_data'] == 'tr' and own['--threshold_from_train'] and rest == ['x.yaml', '--fusion', '--open_set']


def test_without_fusion_parse_own_returns_what_it_returned():
    from opental_amd.common.score_checkpoints import parse_own
    own, rest = parse_own(BASE + ['--open_set', '--split', '1', '--epochs_are_not_mine', '--random_init'])
    assert rest == ['x.yaml', '--open_set', '--split', '1', '--epochs_are_not_mine']
    assert own == {'--random_init': True, '--open_metrics': False, '--threshold_from_train': False, '--wi': False,
                   '--gt': 'gt.json', '--known': 'known.txt', '--ood_threshold': None, '--select': 'average_mAP',
                   '--threshold_videos': None}
    own, rest = parse_own(BASE + ['--open_set', '--open_metrics', '--ood_threshold', '0.25', '--wi', '--select', 'WI'])
    assert own == {'--random_init': False, '--open_metrics': True, '--threshold_from_train': False, '--wi': True,
                   '--gt': 'gt.json', '--known': 'known.txt', '--ood_threshold': 0.25, '--select': 'WI',
                   '--threshold_videos': None}
    assert rest == ['x.yaml', '--open_set']


def test_anet_driver_refuses_fusion():
    from opental_amd.anet.score_checkpoints import main
    with pytest.raises(SystemExit) as e:
        main(BASE + PARTNER)
    assert 'ActivityNet' in str(e.value) and 'no flow stream' in str(e.value) and '--fusion' in str(e.value)


def test_a_recipe_without_a_second_stream_refuses_fusion(tmp_path):
    """The shared driver's own guard (a Recipe without partner_build / fusion_table), after the config is read."""
    import os
    import shutil
    from opental_amd.common.score_checkpoints import Recipe, run
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    yaml_path = str(tmp_path / "c.yaml")
    shutil.copy(os.path.join(repo, "configs", "thumos14_opental_final.yaml"), yaml_path)
    recipe = Recipe('thumos14', ['test'], [0.5], None, None, None, None)
    with pytest.raises(SystemExit) as e:
        run(recipe, [yaml_path, '--gt', 'gt.json', '--known', 'known.txt'] + PARTNER)
    assert 'no second stream' in str(e.value)


def test_held_entries_are_tied_to_their_partner():
    from opental_amd.common.score_checkpoints import holds, merge_entry
    plain = {'mAP': [0.1, 0.2], 'average_mAP': 0.15}
    fused = dict(plain, partner_checkpoint='flow/checkpoint-16.ckpt')
    assert holds(plain, False, None) and not holds(plain, False, None, partner='flow/checkpoint-16.ckpt')
    assert holds(fused, False, None, partner='flow/checkpoint-16.ckpt')
    assert not holds(fused, False, None, partner='flow/checkpoint-17.ckpt')
    assert not holds(fused, False, None)                    # an entry that names a partner is no single-stream entry
    open_lists = dict(AUROC=[0.5], AUPR=[0.5], FAR95=[0.5], OSDR=[0.5], ood_threshold=0.3)
    fused_open = dict(fused, **open_lists)
    assert holds(fused_open, True, 0.3, partner='flow/checkpoint-16.ckpt')
    assert not holds(fused_open, True, 0.4, partner='flow/checkpoint-16.ckpt')          # the threshold rule still holds
    assert not holds(fused_open, True, 0.3, wi=True, partner='flow/checkpoint-16.ckpt')
    assert not holds(fused_open, True, 0.3, partner='flow/checkpoint-17.ckpt')
    assert merge_entry(fused, dict(plain, partner_checkpoint='b'))['partner_checkpoint'] == 'b'


def test_the_two_files_have_different_names():
    from opental_amd.common import score_checkpoints as S
    assert S.MAP_FILE == 'checkpoint_map.json' and S.FUSION_MAP_FILE == 'checkpoint_map_fusion.json'

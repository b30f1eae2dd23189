"""CPU: the host logic of common/score_checkpoints.py -- the command line, the checkpoint list, the best epoch and its ties,
and the refusals that come before any GPU work."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_take_values_and_checkpoint_list(tmp_path):
    from opental_amd.common.score_checkpoints import list_checkpoints, take_values
    argv = ['a.yaml', '--epochs', '3', '12', '--open_set', '--tious', '0.5']
    epochs, rest = take_values(argv, '--epochs')
    assert epochs == ['3', '12'] and rest == ['a.yaml', '--open_set', '--tious', '0.5']
    tious, rest = take_values(rest, '--tious')
    assert tious == ['0.5'] and rest == ['a.yaml', '--open_set']
    assert take_values(rest, '--epochs') == (None, rest)
    for name in ("checkpoint-12.ckpt", "checkpoint-3.ckpt", "checkpoint-latest.ckpt", "checkpoint_map.json", "checkpoint-4.ckpt.tmp"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "training").mkdir()
    (tmp_path / "training" / "checkpoint_7.ckpt").write_bytes(b"")
    found = list_checkpoints(str(tmp_path))
    assert list(found) == [3, 12] and found[12] == str(tmp_path / "checkpoint-12.ckpt")         # by epoch, not by name
    assert list(list_checkpoints(str(tmp_path), [12])) == [12]
    with pytest.raises(FileNotFoundError):
        list_checkpoints(str(tmp_path), [3, 4])
    assert list_checkpoints(str(tmp_path / "nowhere")) == {}


def test_best_epoch_ties_go_to_the_earlier_epoch():
    from opental_amd.common.score_checkpoints import best_epoch
    s = lambda x: {"mAP": [x], "average_mAP": x}
    assert best_epoch({}) is None
    assert best_epoch({"10": s(0.5), "2": s(0.5), "3": s(0.4), "best": 10}) == 2        # numeric order, not the strings'
    assert best_epoch({"1": s(0.1), "2": s(0.3), "3": s(0.3)}) == 2
    assert best_epoch({"1": s(0.0), "2": s(0.0)}) == 1


def test_refusals_come_before_any_gpu_work(tmp_path, monkeypatch):
    """--epochs naming a missing checkpoint, a --known file of another class count, missing --gt, WORLD_SIZE > 1."""
    from make_synthetic_thumos import make
    from opental_amd.common import score_checkpoints as common
    from opental_amd.thumos14 import score_checkpoints as S
    monkeypatch.setattr(common, "device_setup", lambda: pytest.fail("refused runs do not touch the device"))
    yaml_path = make(str(tmp_path / "data"), videos=1, frames=20, size=16, test_videos=1)
    run_dir = tmp_path / "run"
    run_dir.mkdir()
    (run_dir / "checkpoint-3.ckpt").write_bytes(b"")
    gt_file, known = str(tmp_path / "data" / "gt_open.json"), str(tmp_path / "data" / "classes.txt")
    argv = [yaml_path, '--open_set', '--split', '0', '--checkpoint_path', str(run_dir), '--gt', gt_file, '--known', known]
    with pytest.raises(FileNotFoundError):
        S.main(argv + ['--epochs', '3', '4'])
    short = tmp_path / "short.txt"
    short.write_text("7 BaseballPitch\n")
    with pytest.raises(SystemExit, match="classes"):
        S.main(argv[:-1] + [str(short), '--epochs', '3', '--tious', '0.5'])
    with pytest.raises(SystemExit, match="--gt"):
        S.main(argv[:6])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        S.main(argv)
    assert not (run_dir / "checkpoint_map.json").exists()

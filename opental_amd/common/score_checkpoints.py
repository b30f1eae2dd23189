"""Which saved epoch is best: the mAP of every `checkpoint-<epoch>.ckpt` under training.checkpoint_path, on the device.

    python -m opental_amd.thumos14.score_checkpoints <yaml> [--open_set --split N] --gt GT.json --known KNOWN.txt \\
           [--epochs A B ...] [--tious ...] [--random_init] [--select KEY] [--ema] \\
           [--open_metrics [--ood_threshold THR | --threshold_from_train [--threshold_videos N]] [--wi]] \\
           [--fusion --partner_checkpoint PATH --partner_data DIR [--partner_train_data DIR]]
    python -m opental_amd.anet.score_checkpoints     ... the same, with the ActivityNet defaults

The network is built once; per checkpoint its state dict is loaded, the test videos go through the recipe's device pipeline
(thumos14.test.detect_batch / anet.test.detect_rows, with the batches, conf_thresh, top_k and nms_sigma of the recipe's
test.py), every batch's Soft-NMS rows become a detection table (ops.detection_table; the batch's first video's number is added
to its `video` column) and evaluation/table_ap.py turns the tables and the ground truth into AP per class and tIoU.  No
proposal dicts and no result JSON are built; the only reads from the device are one row count per table and the AP array.

One line is printed per epoch and <checkpoint_path>/checkpoint_map.json holds {epoch: {"mAP": [...], "average_mAP": x}, ...,
"best": epoch}; equal averages go to the earlier epoch, and an epoch already in the file is not scored again.  With
--random_init the checkpoints' weights are not loaded (every listed epoch is scored with the network's own initialisation: a
dry run of the pipeline).  One process only; the RPL / GCPL heads and OpenMax are not served.

--fusion (THUMOS14) scores the listed epochs TOGETHER WITH one fixed checkpoint of the other stream: model.in_channels of the
yaml says which stream the epochs under training.checkpoint_path are (3: rgb, 2: flow, with the flow yaml), the partner is
--partner_checkpoint PATH, loaded once into a second network of the other channel count and the same head settings, and its
videos come from --partner_data DIR (for --threshold_from_train from --partner_train_data DIR; no default is guessed).  Every
batch goes through the recipe's two-stream pipeline (thumos14.test.detect_batch with flow_net: the two networks' raw maps in
one decode launch) and everything after the table is what it is single-stream, all flags included.  The results go to
<checkpoint_path>/checkpoint_map_fusion.json -- checkpoint_map.json is neither read nor written -- and every entry records its
"partner_checkpoint": an entry made with another partner does not count as held and is scored again.

--open_metrics (with --open_set) scores every epoch by AUROC, AUPR, FAR@95 and OSDR per tIoU as well, from the same tables
(evaluation/table_open.py; their `known` column follows testing.ood_scoring / --ood_scoring), relabelling detections below
--ood_threshold THR as unknown when it is given.  An epoch's entry gains "AUROC", "AUPR", "FAR95" and "OSDR" lists (NaN written as
null; "ood_threshold" when one was given) and its line their means; an epoch is skipped only when its entry already holds all
that is asked for, otherwise it is scored and the entry merged.  --select KEY names what "best" goes by: average_mAP (default),
AUROC, AUPR, OSDR or FAR95, the mean over the thresholds; FAR95 is best where it is lowest, a NaN mean is never best, equal means
go to the earlier epoch.  Without these flags the output and the file are what they were without them.

--threshold_from_train (with --open_metrics, instead of a numeric --ood_threshold) gives every epoch its OWN known / unknown
operating point, as the protocol does (thumos14/threshold.py, anet/threshold.py): after the state dict is loaded the recipe's
training videos go through the same device pipeline (Recipe.train_table), each table's known[:n] is kept, and
det_table.threshold_from_scores over their concatenation -- the known-ness value that 95 % of the detections exceed -- is the
epoch's ood_threshold for table_open and table_wi.  The entry records it as "ood_threshold" with "ood_threshold_from": "train";
--threshold_videos N caps the pass at the first N training videos (smoke runs) and is recorded as "threshold_videos": an entry
made under another cap, or none, does not count as held.  --wi (with one of the two threshold sources) adds the Wilderness
Impact (evaluation/table_wi.py): "WI", per tIoU the mean over the K classes, NaN as null; the epoch's line gains " WI <mean>"
and, with --threshold_from_train, " thr <value>".  --select WI is best where it is lowest, as FAR95.

--ema scores the averaged models a run with --ema_decay saved, `checkpoint-ema-<epoch>.ckpt` (the same keys as the weights
files), in place of the weights: the results go to <checkpoint_path>/checkpoint_map_ema.json (checkpoint_map_fusion_ema.json
with --fusion) and checkpoint_map.json is neither read nor written.  Every other flag works as before.

A recipe's module hands `run` a Recipe: how to build its network, list its test videos and detect one batch -- and, for
--threshold_from_train, how to list its training videos and detect one batch of them."""
import json
import os
import re
import sys

import numpy as np
import torch

from . import config as C
from .driver import device_setup, split_flags, write_json

MAP_FILE = 'checkpoint_map.json'
FUSION_MAP_FILE = 'checkpoint_map_fusion.json'      # --fusion: its own file, entries tied to their "partner_checkpoint"
PARTNER_OPTIONS = ('--partner_checkpoint', '--partner_data', '--partner_train_data')
OPEN_KEYS = ('AUROC', 'AUPR', 'FAR95', 'OSDR')      # an entry's open-set lists, in the order of table_open.KEYS
SELECT_KEYS = ('average_mAP',) + OPEN_KEYS + ('WI',)
LOWER_IS_BETTER = ('FAR95', 'WI')
THRESHOLD_KEYS = ('ood_threshold', 'ood_threshold_from', 'threshold_videos', 'WI')     # what a scoring at another threshold stales
_CKPT = re.compile(r'^checkpoint-(\d+)\.ckpt$')
_EMA_CKPT = re.compile(r'^checkpoint-ema-(\d+)\.ckpt$')         # --ema: the averaged models (DetectorTrainer.save_model)
EMA_MAP_FILE = 'checkpoint_map_ema.json'
FUSION_EMA_MAP_FILE = 'checkpoint_map_fusion_ema.json'


class Recipe(object):
    """dataset: ANETdetection's dataset name (how the class file is read); subset: the ground truth's subsets; tious: the
    default thresholds; build(config, dev) -> the network, randomly initialised, in eval mode;
    videos(config) -> (names as the ground truth spells them, state); batches(config, state) -> lists of positions into names;
    table(net, config, state, positions, dev, scoring=...) -> the detection table of these videos (video column
    0 .. len(positions)-1), its `known` column by the out-of-distribution score `scoring`.
    Optional, for --threshold_from_train: train_videos(config) -> (names, state) of the TRAINING split, which `batches` cuts
    into batches like the test split's; train_table(net, config, state, positions, dev, scoring=...) -> the same table as
    `table`, over these videos.
    Optional, for --fusion: partner_build(config, dev) -> the network of the OTHER stream (the other channel count, the same
    head settings), randomly initialised, in eval mode; fusion_table(net, partner, partner_data, config, state, positions, dev,
    scoring=..., train=False) -> the table of the two-stream pipeline over these videos, the partner's read from the directory
    `partner_data`; train=True: the listed stream's videos are the training split's, as train_table's."""

    def __init__(self, dataset, subset, tious, build, videos, batches, table, train_videos=None, train_table=None,
                 partner_build=None, fusion_table=None):
        self.dataset, self.subset, self.tious = dataset, subset, tious
        self.build, self.videos, self.batches, self.table = build, videos, batches, table
        self.train_videos, self.train_table = train_videos, train_table
        self.partner_build, self.fusion_table = partner_build, fusion_table

    def with_partner(self, partner, partner_data, partner_train_data):
        """This recipe with `table` / `train_table` made by the two-stream pipeline with the network `partner`."""
        table = lambda net, *a, **kw: self.fusion_table(net, partner, partner_data, *a, **kw)
        train_table = lambda net, *a, **kw: self.fusion_table(net, partner, partner_train_data, *a, train=True, **kw)
        return Recipe(self.dataset, self.subset, self.tious, self.build, self.videos, self.batches, table, self.train_videos,
                      train_table)


def take_values(argv, flag):
    """`flag A B ...` taken out of a command line: the values up to the next --option (None without the flag), the rest."""
    if flag not in argv:
        return None, list(argv)
    i = argv.index(flag)
    j = i + 1
    while j < len(argv) and not argv[j].startswith('--'):
        j += 1
    return argv[i + 1:j], argv[:i] + argv[j:]


def list_checkpoints(checkpoint_path, epochs=None, ema=False):
    """{epoch: path} of the checkpoint-<epoch>.ckpt files of a directory (ema: the checkpoint-ema-<epoch>.ckpt ones),
    ascending; `epochs`: only these, all of which must exist."""
    found = {}
    for f in os.listdir(checkpoint_path) if os.path.isdir(checkpoint_path) else []:
        m = (_EMA_CKPT if ema else _CKPT).match(f)
        if m:
            found[int(m.group(1))] = os.path.join(checkpoint_path, f)
    if epochs is not None:
        missing = [e for e in epochs if e not in found]
        if missing:
            raise FileNotFoundError("no checkpoint-%s<epoch>.ckpt under %s for epoch(s) %s"
                                    % ("ema-" if ema else "", checkpoint_path, missing))
        found = {e: found[e] for e in epochs}
    return dict(sorted(found.items()))


def select_value(entry, key):
    """What --select KEY compares: the entry's average_mAP, or the mean of its KEY list over the thresholds (null = NaN),
    negated for FAR95 and WI so that larger is better throughout.  None where the entry does not hold the key."""
    if key == 'average_mAP':
        return entry.get('average_mAP')
    values = entry.get(key)
    if values is None:
        return None
    mean = float(np.mean([np.nan if v is None else v for v in values])) if len(values) else float('nan')
    return -mean if key in LOWER_IS_BETTER else mean


def best_epoch(scores, key='average_mAP'):
    """The epoch of the largest average_mAP (or of the best `key`, select_value); equal values go to the earlier epoch, an
    epoch without the key or with a NaN mean is never best.  None without such epochs."""
    best, best_value = None, None
    for e in sorted(int(k) for k in scores if k != 'best'):
        value = select_value(scores[str(e)], key)
        if value is None or value != value:
            continue
        if best is None or value > best_value:
            best, best_value = e, value
    return best


def holds(entry, open_metrics, ood_threshold, wi=False, from_train=False, threshold_videos=None, partner=None):
    """Whether an epoch's entry already holds everything asked for: the mAP, and with `open_metrics` the four lists, scored
    with this ood_threshold -- or, with `from_train`, with the epoch's own threshold from the training split under this
    `threshold_videos` cap; with `wi` the "WI" list too.  partner (--fusion): the entry must have been made with this
    partner checkpoint; without it an entry that names a partner does not count either."""
    if 'mAP' not in entry or 'average_mAP' not in entry or entry.get('partner_checkpoint') != partner:
        return False
    if not open_metrics:
        return True
    if not all(k in entry for k in OPEN_KEYS) or (wi and 'WI' not in entry):
        return False
    if from_train:
        return entry.get('ood_threshold_from') == 'train' and entry.get('ood_threshold') is not None \
            and entry.get('threshold_videos') == threshold_videos
    return entry.get('ood_threshold') == ood_threshold and 'ood_threshold_from' not in entry


def merge_entry(old, new):
    """The entry after a scoring: the old one's keys, replaced by the new one's; an ood_threshold, where it came from and the
    WI scored at it only where the new one has them."""
    return dict({k: v for k, v in (old or {}).items() if k not in THRESHOLD_KEYS}, **new)


def open_entry(metrics, ood_threshold, wi=None, from_train=False, threshold_videos=None):
    """table_open's result as an entry's lists: NaN as None (null in the file).  wi: table_wi's (nthr, K) array, recorded as
    "WI", its mean over the classes per tIoU; from_train / threshold_videos: where the ood_threshold came from."""
    from ..evaluation.table_open import KEYS
    entry = {name: [None if v != v else float(v) for v in metrics[k]] for name, k in zip(OPEN_KEYS, KEYS)}
    if ood_threshold is not None:
        entry['ood_threshold'] = ood_threshold
    if from_train:
        entry['ood_threshold_from'] = 'train'
        if threshold_videos is not None:
            entry['threshold_videos'] = threshold_videos
    if wi is not None:
        entry['WI'] = [None if v != v else float(v) for v in np.asarray(wi, dtype=np.float64).mean(axis=1)]
    return entry


def parse_own(argv):
    """The driver's own arguments: (own, rest).  own['--ood_threshold'] is a float or None, own['--threshold_videos'] an int
    or None.  --fusion stays in `rest` (the config parser knows it: testing.fusion); with it own holds the PARTNER_OPTIONS."""
    own, rest = split_flags(argv, ('--random_init', '--open_metrics', '--threshold_from_train', '--wi'),
                            {'--gt': (1, None), '--known': (1, None), '--ood_threshold': (1, None), '--select': (1, 'average_mAP'),
                             '--threshold_videos': (1, None), **{name: (1, None) for name in PARTNER_OPTIONS}})
    partner = {name: own.pop(name) for name in PARTNER_OPTIONS}
    if '--fusion' in rest:
        for name in PARTNER_OPTIONS[:2]:
            if partner[name] is None:
                raise SystemExit("score_checkpoints: --fusion needs %s: the other stream's %s (no default is guessed)"
                                 % (name, "checkpoint" if name == '--partner_checkpoint' else "test videos"))
        if own['--threshold_from_train'] and partner['--partner_train_data'] is None:
            raise SystemExit("score_checkpoints: --fusion with --threshold_from_train needs --partner_train_data: the other "
                             "stream's training videos (no default is guessed)")
        own.update(partner)
    else:
        given = [name for name in PARTNER_OPTIONS if partner[name] is not None]
        if given:
            raise SystemExit("score_checkpoints: %s belong%s to a two-stream run: add --fusion"
                             % (", ".join(given), "s" if len(given) == 1 else ""))
    if own['--gt'] is None or own['--known'] is None:
        raise SystemExit("score_checkpoints: --gt GT.json and --known KNOWN.txt are required")
    if own['--select'] not in SELECT_KEYS:
        raise SystemExit("score_checkpoints: --select takes one of %s" % ", ".join(SELECT_KEYS))
    if own['--open_metrics'] and '--open_set' not in rest:
        raise SystemExit("score_checkpoints: --open_metrics belongs to the open-set protocol: add --open_set")
    if not own['--open_metrics'] and (own['--select'] in OPEN_KEYS or own['--ood_threshold'] is not None):
        raise SystemExit("score_checkpoints: --select %s and --ood_threshold need --open_metrics" % "/".join(OPEN_KEYS))
    if not own['--open_metrics'] and (own['--threshold_from_train'] or own['--wi']):
        raise SystemExit("score_checkpoints: --threshold_from_train and --wi need --open_metrics")
    if own['--threshold_from_train'] and own['--ood_threshold'] is not None:
        raise SystemExit("score_checkpoints: --threshold_from_train and a numeric --ood_threshold exclude each other")
    if own['--threshold_videos'] is not None and not own['--threshold_from_train']:
        raise SystemExit("score_checkpoints: --threshold_videos caps the pass of --threshold_from_train")
    if own['--wi'] and not own['--threshold_from_train'] and own['--ood_threshold'] is None:
        raise SystemExit("score_checkpoints: --wi needs a threshold: --ood_threshold THR or --threshold_from_train")
    if own['--select'] == 'WI' and not own['--wi']:
        raise SystemExit("score_checkpoints: --select WI needs --wi")
    if own['--ood_threshold'] is not None:
        own['--ood_threshold'] = float(own['--ood_threshold'])
    if own['--threshold_videos'] is not None:
        own['--threshold_videos'] = int(own['--threshold_videos'])
        if own['--threshold_videos'] < 1:
            raise SystemExit("score_checkpoints: --threshold_videos takes a positive number of videos")
    return own, rest


def read_map(path):
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return {k: v for k, v in json.load(f).items() if k != 'best'}


def epoch_tables(recipe, net, config, state, batches, dev, scoring=None):
    """The detection tables of one pass over the test videos, videos numbered by their position in the recipe's list.
    scoring: the out-of-distribution score behind the tables' `known` column (None: the recipe's default)."""
    tables = []
    kw = {} if scoring is None else dict(scoring=scoring)
    with torch.no_grad():
        for part in batches:
            table = recipe.table(net, config, state, part, dev, **kw)
            table['video'] += part[0]           # a batch holds consecutive videos
            tables.append(table)
    return tables


def train_threshold(recipe, net, config, state, batches, dev, scoring=None):
    """The epoch's own known / unknown operating point: the training videos through Recipe.train_table batch by batch, each
    table's known[:n] kept (one host read per table), det_table.threshold_from_scores over their concatenation."""
    from .det_table import threshold_from_scores
    parts = []
    kw = {} if scoring is None else dict(scoring=scoring)
    with torch.no_grad():
        for part in batches:
            table = recipe.train_table(net, config, state, part, dev, **kw)
            parts.append(table['known'][:int(table['n'])].clone())         # the table itself is sized for the upper bound
    return threshold_from_scores(torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float64))


def capped(batches, cap):
    """The batches over the first `cap` videos only (None: all of them)."""
    if cap is None:
        return batches
    return [part for part in ([p for p in part if p < cap] for part in batches) if part]


def run(recipe, argv=None):
    """The driver.  Returns (the path of checkpoint_map.json -- checkpoint_map_fusion.json with --fusion --, its content)."""
    from ..evaluation.table_ap import GroundTruth, table_ap
    argv = list(sys.argv[1:] if argv is None else argv)
    epochs, argv = take_values(argv, '--epochs')
    tious, argv = take_values(argv, '--tious')
    ema, argv = '--ema' in argv, [a for a in argv if a != '--ema']     # the averaged models, into a map file of their own
    own, rest = parse_own(argv)
    open_metrics, ood_threshold, select = own['--open_metrics'], own['--ood_threshold'], own['--select']
    from_train, cap, want_wi = own['--threshold_from_train'], own['--threshold_videos'], own['--wi']
    if from_train and (recipe.train_videos is None or recipe.train_table is None):
        raise SystemExit("score_checkpoints: this recipe does not list its training videos: --threshold_from_train is not served")
    if int(os.environ.get('WORLD_SIZE', 1)) > 1:
        raise SystemExit("score_checkpoints runs in one process (WORLD_SIZE > 1 is not served): start it without torchrun")
    config = C.set_config(C.get_config(rest))
    fusion = bool(config['testing'].get('fusion', False))
    if config['model'].get('use_rpl', False):
        raise SystemExit("score_checkpoints: the RPL / GCPL heads are not served")
    if fusion and (recipe.partner_build is None or recipe.fusion_table is None):
        raise SystemExit("score_checkpoints: this recipe has no second stream: --fusion is not served")
    partner_path = own['--partner_checkpoint'] if fusion else None
    tious = np.asarray(recipe.tious if tious is None else [float(t) for t in tious], dtype=np.float64)
    ckpt_dir = config['training']['checkpoint_path']
    ckpts = list_checkpoints(ckpt_dir, None if epochs is None else [int(e) for e in epochs], ema=ema)
    if ema:
        map_file = os.path.join(ckpt_dir, FUSION_EMA_MAP_FILE if fusion else EMA_MAP_FILE)
    else:
        map_file = os.path.join(ckpt_dir, FUSION_MAP_FILE if fusion else MAP_FILE)
    scores = read_map(map_file)
    todo = {e: p for e, p in ckpts.items()
            if str(e) not in scores or not holds(scores[str(e)], open_metrics, ood_threshold, want_wi, from_train, cap,
                                                 partner_path)}
    for e in ckpts:
        if e not in todo:
            print(f"epoch {e}: already in {map_file}, skipped")
    if todo:
        check_classes(config, own['--known'], recipe.dataset)
        _, _, dev = device_setup()
        names, state = recipe.videos(config)
        gt = GroundTruth.load(own['--gt'], own['--known'], subset=recipe.subset, dataset=recipe.dataset, videos=names)
        net = recipe.build(config, dev)
        if fusion:
            partner = recipe.partner_build(config, dev)
            if not own['--random_init']:
                partner.load_state_dict(torch.load(partner_path, map_location='cpu'))
            recipe = recipe.with_partner(partner, own['--partner_data'], own['--partner_train_data'])
        batches = recipe.batches(config, state)
        if from_train:
            _, train_state = recipe.train_videos(config)
            train_batches = capped(recipe.batches(config, train_state), cap)
        for e, path in todo.items():
            if not own['--random_init']:
                net.load_state_dict(torch.load(path, map_location='cpu'))
            if from_train:
                ood_threshold = train_threshold(recipe, net, config, train_state, train_batches, dev,
                                                config['testing']['ood_scoring'])
            tables = epoch_tables(recipe, net, config, state, batches, dev,
                                  config['testing']['ood_scoring'] if open_metrics else None)
            ap = table_ap(tables, gt, tious)
            mAP = ap.mean(axis=1)
            entry = {"mAP": mAP.tolist(), "average_mAP": float(mAP.mean())}
            line = f"epoch {e}: " + " ".join(f"mAP@{t:.2f} {m:.4f}" for t, m in zip(tious, mAP)) + f" average {mAP.mean():.4f}"
            if open_metrics:
                from ..evaluation.table_open import KEYS, table_open
                metrics = table_open(tables, gt, tious, ood_threshold)
                wi = None
                if want_wi:
                    from ..evaluation.table_wi import table_wi
                    wi = table_wi(tables, gt, tious, ood_threshold)
                entry.update(open_entry(metrics, ood_threshold, wi, from_train, cap))
                line += "".join(f" {name} {np.mean(metrics[k]):.4f}" for name, k in zip(OPEN_KEYS, KEYS))
                if want_wi:
                    line += f" WI {wi.mean():.4f}"
                if from_train:
                    line += f" thr {ood_threshold:.6f}"
            old = scores.get(str(e))
            if fusion:
                entry['partner_checkpoint'] = partner_path
                if old is not None and old.get('partner_checkpoint') != partner_path:
                    old = None                  # scored with another partner: nothing of it carries over
            scores[str(e)] = merge_entry(old, entry)
            print(line)
            write_json(map_file, dict(scores, best=best_epoch(scores, select)))
    result = dict(scores, best=best_epoch(scores, select))
    print(f"best epoch: {result['best']} -> {map_file}")
    return map_file, result


def check_classes(config, known, dataset):
    """A table's class c is the network's class c + 1, named by line c of dataset.class_info_path; AP column c is line c of
    the --known file.  The two must be the same list (the recipes' split files are)."""
    from ..evaluation.table_ap import class_names
    names = class_names(known, dataset)
    if len(names) != int(config['dataset']['num_classes']) - 1:
        raise SystemExit("score_checkpoints: the network has %d classes, %s names %d"
                         % (int(config['dataset']['num_classes']) - 1, known, len(names)))
    path = config['dataset'].get('class_info_path')
    if path and os.path.exists(path) and class_names(path, dataset) != names:
        raise SystemExit("score_checkpoints: %s and %s list different classes" % (path, known))

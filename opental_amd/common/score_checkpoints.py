"""Which saved epoch is best: the mAP of every `checkpoint-<epoch>.ckpt` under training.checkpoint_path, on the device.

    python -m opental_amd.thumos14.score_checkpoints <yaml> [--open_set --split N] --gt GT.json --known KNOWN.txt \\
           [--epochs A B ...] [--tious ...] [--random_init]
    python -m opental_amd.anet.score_checkpoints     ... the same, with the ActivityNet defaults

The network is built once; per checkpoint its state dict is loaded, the test videos go through the recipe's device pipeline
(thumos14.test.detect_batch / anet.test.detect_rows, with the batches, conf_thresh, top_k and nms_sigma of the recipe's
test.py), every batch's Soft-NMS rows become a detection table (ops.detection_table; the batch's first video's number is added
to its `video` column) and evaluation/table_ap.py turns the tables and the ground truth into AP per class and tIoU.  No
proposal dicts and no result JSON are built; the only reads from the device are one row count per table and the AP array.

One line is printed per epoch and <checkpoint_path>/checkpoint_map.json holds {epoch: {"mAP": [...], "average_mAP": x}, ...,
"best": epoch}; equal averages go to the earlier epoch, and an epoch already in the file is not scored again.  With
--random_init the checkpoints' weights are not loaded (every listed epoch is scored with the network's own initialisation: a
dry run of the pipeline).  One process only; two-stream fusion, the RPL / GCPL heads and OpenMax are not served.

A recipe's module hands `run` a Recipe: how to build its network, list its test videos and detect one batch."""
import json
import os
import re
import sys

import numpy as np
import torch

from . import config as C
from .driver import device_setup, split_flags, write_json

MAP_FILE = 'checkpoint_map.json'
_CKPT = re.compile(r'^checkpoint-(\d+)\.ckpt$')


class Recipe(object):
    """dataset: ANETdetection's dataset name (how the class file is read); subset: the ground truth's subsets; tious: the
    default thresholds; build(config, dev) -> the network, randomly initialised, in eval mode;
    videos(config) -> (names as the ground truth spells them, state); batches(config, state) -> lists of positions into names;
    table(net, config, state, positions, dev) -> the detection table of these videos (video column 0 .. len(positions)-1)."""

    def __init__(self, dataset, subset, tious, build, videos, batches, table):
        self.dataset, self.subset, self.tious = dataset, subset, tious
        self.build, self.videos, self.batches, self.table = build, videos, batches, table


def take_values(argv, flag):
    """`flag A B ...` taken out of a command line: the values up to the next --option (None without the flag), the rest."""
    if flag not in argv:
        return None, list(argv)
    i = argv.index(flag)
    j = i + 1
    while j < len(argv) and not argv[j].startswith('--'):
        j += 1
    return argv[i + 1:j], argv[:i] + argv[j:]


def list_checkpoints(checkpoint_path, epochs=None):
    """{epoch: path} of the checkpoint-<epoch>.ckpt files of a directory, ascending; `epochs`: only these, all of which
    must exist."""
    found = {}
    for f in os.listdir(checkpoint_path) if os.path.isdir(checkpoint_path) else []:
        m = _CKPT.match(f)
        if m:
            found[int(m.group(1))] = os.path.join(checkpoint_path, f)
    if epochs is not None:
        missing = [e for e in epochs if e not in found]
        if missing:
            raise FileNotFoundError("no checkpoint-<epoch>.ckpt under %s for epoch(s) %s" % (checkpoint_path, missing))
        found = {e: found[e] for e in epochs}
    return dict(sorted(found.items()))


def best_epoch(scores):
    """The epoch of the largest average_mAP; equal values go to the earlier epoch.  None without epochs."""
    best = None
    for e in sorted(int(k) for k in scores if k != 'best'):
        if best is None or scores[str(e)]['average_mAP'] > scores[str(best)]['average_mAP']:
            best = e
    return best


def read_map(path):
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return {k: v for k, v in json.load(f).items() if k != 'best'}


def epoch_tables(recipe, net, config, state, batches, dev):
    """The detection tables of one pass over the test videos, videos numbered by their position in the recipe's list."""
    tables = []
    with torch.no_grad():
        for part in batches:
            table = recipe.table(net, config, state, part, dev)
            table['video'] += part[0]           # a batch holds consecutive videos
            tables.append(table)
    return tables


def run(recipe, argv=None):
    """The driver.  Returns (the path of checkpoint_map.json, its content)."""
    from ..evaluation.table_ap import GroundTruth, table_ap
    argv = list(sys.argv[1:] if argv is None else argv)
    epochs, argv = take_values(argv, '--epochs')
    tious, argv = take_values(argv, '--tious')
    own, rest = split_flags(argv, ('--random_init',), {'--gt': (1, None), '--known': (1, None)})
    if own['--gt'] is None or own['--known'] is None:
        raise SystemExit("score_checkpoints: --gt GT.json and --known KNOWN.txt are required")
    if int(os.environ.get('WORLD_SIZE', 1)) > 1:
        raise SystemExit("score_checkpoints runs in one process (WORLD_SIZE > 1 is not served): start it without torchrun")
    config = C.set_config(C.get_config(rest))
    if config['testing'].get('fusion', False) or config['model'].get('use_rpl', False):
        raise SystemExit("score_checkpoints: two-stream fusion and the RPL / GCPL heads are not served")
    tious = np.asarray(recipe.tious if tious is None else [float(t) for t in tious], dtype=np.float64)
    ckpt_dir = config['training']['checkpoint_path']
    ckpts = list_checkpoints(ckpt_dir, None if epochs is None else [int(e) for e in epochs])
    map_file = os.path.join(ckpt_dir, MAP_FILE)
    scores = read_map(map_file)
    todo = {e: p for e, p in ckpts.items() if str(e) not in scores}
    for e in ckpts:
        if e not in todo:
            print(f"epoch {e}: already in {map_file}, skipped")
    if todo:
        check_classes(config, own['--known'], recipe.dataset)
        _, _, dev = device_setup()
        names, state = recipe.videos(config)
        gt = GroundTruth.load(own['--gt'], own['--known'], subset=recipe.subset, dataset=recipe.dataset, videos=names)
        net = recipe.build(config, dev)
        batches = recipe.batches(config, state)
        for e, path in todo.items():
            if not own['--random_init']:
                net.load_state_dict(torch.load(path, map_location='cpu'))
            ap = table_ap(epoch_tables(recipe, net, config, state, batches, dev), gt, tious)
            mAP = ap.mean(axis=1)
            scores[str(e)] = {"mAP": mAP.tolist(), "average_mAP": float(mAP.mean())}
            print(f"epoch {e}: " + " ".join(f"mAP@{t:.2f} {m:.4f}" for t, m in zip(tious, mAP)) + f" average {mAP.mean():.4f}")
            write_json(map_file, dict(scores, best=best_epoch(scores)))
    result = dict(scores, best=best_epoch(scores))
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

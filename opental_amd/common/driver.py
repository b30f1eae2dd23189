"""What the `main`s of the inference drivers share (thumos14/test.py, test_openmax.py, test_cross_data.py, threshold.py,
anet/test.py, anet/threshold.py): their own command-line flags, the device of this rank, the network with its checkpoint,
and the result file."""
import json
import os

import torch


def split_flags(argv, flags=(), options=None):
    """The drivers' own arguments taken out of a command line; the rest goes to the config parser.  flags: names that
    stand alone (--random_init).  options: {name: (number of values, default)} (--evaluate A B).  Returns (found, rest):
    found[name] is True / False for a flag; for an option the value that followed it (a tuple of them when it takes
    several) or its default."""
    options = options or {}
    found = {f: False for f in flags}
    found.update({name: default for name, (_, default) in options.items()})
    rest, i = [], 0
    while i < len(argv):
        a = argv[i]
        if a in flags:
            found[a] = True
        elif a in options:
            n = options[a][0]
            values = tuple(argv[i + 1:i + 1 + n])
            if len(values) < n:
                raise ValueError(f"{a} takes {n} value{'s' if n > 1 else ''}, {len(values)} given")
            found[a] = values[0] if n == 1 else values
            i += n
        else:
            rest.append(a)
        i += 1
    return found, rest


def device_setup():
    """(rank, world, device) of this process under torchrun (one process, device 0, without it).  Makes the device current
    and sets the convolutions' precision from OTAL_DTYPE (bf16 operands unless it says otherwise)."""
    from . import ops
    rank, world = int(os.environ.get('RANK', 0)), int(os.environ.get('WORLD_SIZE', 1))
    dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', 0)))
    torch.cuda.set_device(dev)
    ops.CONV_PRECISION = 1 if os.environ.get('OTAL_DTYPE', 'bf16') == 'bf16' else 0
    return rank, world, dev


def load_net(BDNet, dev, random_init, checkpoint_path, **bdnet_kwargs):
    """BDNet(training=False, **bdnet_kwargs) with the checkpoint's weights (its own initialisation with `random_init`), on
    the device, in eval mode."""
    net = BDNet(training=False, **bdnet_kwargs)
    if not random_init:
        net.load_state_dict(torch.load(checkpoint_path, map_location='cpu'))
    return net.to(dev).eval()


def write_json(path, obj):
    """Written under a temporary name of this process next to its place and moved in (os.replace is atomic), so that a
    reader, or a later run looking for a file to re-use, never sees half a file."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, 'w') as f:
        json.dump(obj, f)
    os.replace(tmp, path)

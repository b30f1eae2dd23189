"""Records every max-pool, GroupNorm and glue call of the model's workloads, for tests/test_layer_calls_gpu.py.

    python tools/record_layer_calls.py record OUT.npz     # on the GPU: every call -> OUT.npz, distinct ones -> the golden file
    python tools/record_layer_calls.py pool_choice OUT.npz   # on the GPU: the kernel every pool item of the test gets

`record` runs what tools/record_conv_calls.py runs -- one eager THUMOS14 training step at b = 8 and at b = 1, one ActivityNet
step at b = 2 and one inference batch (bench.py's models, synthetic clips, bf16 operands) -- and a second THUMOS14 step at b = 8
with ops.HALF_CHAIN and ops.HALF_STORAGE off, which takes the fp32 pool entry points (out_mask, fp32 sign bits).  Per call it
keeps the entry point, the integer arguments in the layout of oracle.layer_ref.FIELDS (geometry, strides, io bits, nonneg,
accumulate, which nullable operands were given, summed terms, level table), GroupNorm's eps, and each pointer's address
mod 16 in the order of oracle.layer_ref.ADDRS.  tests/golden/layer_calls.npz keeps one row per distinct call, from the first
workload that made it.

`pool_choice` is the fixture of tests/test_pool_select_cpu.py (tests/golden/pool_choice.npz): it makes every pool item of
tests/test_layer_calls_gpu.py -- the recorded rows, their variants, pool_extra() and the documented refusals -- exactly as
the test makes it (the test's own functions, value checks included) and keeps per item the label, the family, the integer
columns of FIELDS as passed after the variant, the five address residues, the switches set, the return code and
otal_layer_last_kernel().  Record it with the library whose choice is to be pinned, BEFORE a change to the selection (the
test's functions also hold every answer against the CPU harness of the working tree, so the two must agree at that point).
"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden", "layer_calls.npz")

from oracle.layer_ref import FIELDS, NINTS  # noqa: E402


def _v(p):
    """A pointer / integer argument as a Python int (0 for NULL)."""
    if isinstance(p, ctypes.c_void_p):
        return int(p.value or 0)
    if p is None:
        return 0
    return int(p)


def _a(p):
    return _v(p) % 16


def _arr(a, n):
    """The first n entries of a ctypes array argument (pointers: 0 for NULL)."""
    return [int(v or 0) for v in list(a)[:n]]


def _lev(nlev, lev):
    vals = _arr(lev, nlev + 1) if (lev is not None and nlev > 1) else []
    return vals + [0] * (9 - len(vals))


def _pool_fwd(name, a):
    geom, strides = _arr(a[0], 17), _arr(a[1], 4)
    x, y, arg = a[2], a[3], a[4]
    bits = a[5] if name in ("otal_maxpool3d_fwd_signbits", "otal_maxpool3d_fwd_signbits_h", "otal_maxpool3d_fwd_io") else None
    io = {"otal_maxpool3d_fwd": 0, "otal_maxpool3d_fwd_signbits": 0, "otal_maxpool3d_fwd_signbits_h": 1}.get(name)
    if io is None:
        io = int(a[6])
    ints = geom + strides + [io & 3, (io >> 2) & 1, int(_v(bits) != 0)]
    return ints, 0.0, [_a(x), _a(y), _a(arg), _a(bits), 0]


def _pool_bwd(name, a):
    geom, strides = _arr(a[0], 17), _arr(a[1], 4)
    dy, arg, dx = a[2], a[3], a[4]
    if name == "otal_maxpool3d_bwd":
        acc, mask, scale, bits, io = a[5], a[6], a[7], None, 0
    elif name == "otal_maxpool3d_bwd_signbits":
        acc, mask, scale, bits, io = a[5], None, a[7], a[6], 0
    elif name == "otal_maxpool3d_bwd_signbits_h":
        acc, mask, scale, bits, io = 0, None, a[6], a[5], 1
    else:
        acc, mask, scale, bits, io = a[5], a[6], a[7], a[8], int(a[9])
    ints = geom + strides + [io, int(acc), int(_v(mask) != 0), int(_v(scale) != 0), int(_v(bits) != 0)]
    return ints, 0.0, [_a(dy), _a(dx), _a(arg), _a(bits), _a(mask)]


def _gn_fwd(name, a):
    pair, to = "pair" in name, name.endswith("_to")
    x, gamma, beta, y = a[0], a[1], a[2], a[3]
    k = 4
    y_bs = y_cs = 0
    if to:
        y_bs, y_cs = _v(a[4]), _v(a[5])
        k = 6
    stats = a[k]
    B, C, T, G, eps, relu, nlev, lev = a[k + 1:k + 9]
    first = (lambda p: _arr(p, 1)[0]) if pair else _v
    ints = [B, C, T, G, int(relu), int(pair), y_bs, y_cs, int(nlev)] + _lev(int(nlev), lev)
    return ints, float(eps), [_a(first(x)), _a(first(y)), _a(first(stats)), 0, 0]


def _gn_bwd(name, a):
    terms = [(0, 0, 0)] * 3
    if name == "otal_gn_relu_bwd_sum":
        n = int(a[0])
        ptrs, bs, cs, tt = _arr(a[1], n), _arr(a[2], n), _arr(a[3], n), _arr(a[4], n)
        terms = [(bs[i], cs[i], tt[i]) for i in range(n)] + [(0, 0, 0)] * (3 - n)
        x, dx = a[5], a[9]
        B, C, T, G, relu, nlev, lev = a[11:18]
        addrs = [p % 16 for p in ptrs] + [0] * (3 - n) + [_a(x), _a(dx)]
        pair, dy_bs = 0, 0
    elif name == "otal_gn_relu_bwd_pair":
        n, pair = 0, 1
        dy_bs = _arr(a[1], 2)[0]
        B, C, T, G, relu, nlev, lev = a[8:15]
        addrs = [_arr(a[0], 1)[0] % 16, 0, 0, _arr(a[2], 1)[0] % 16, _arr(a[6], 1)[0] % 16]
    else:
        n, pair = 0, 0
        dy_bs = _v(a[1])
        B, C, T, G, relu, nlev, lev = a[8:15]
        addrs = [_a(a[0]), 0, 0, _a(a[2]), _a(a[6])]
    ints = [B, C, T, G, int(relu), pair, int(nlev)] + _lev(int(nlev), lev) + [dy_bs, n] + [v for t in terms for v in t]
    return ints, 0.0, addrs


def _sum_partials(name, a):
    n = int(a[0])
    cs, bs = _arr(a[5], n), _arr(a[6], n)
    ints = [n] + [v for c, b in list(zip(cs, bs))[:32] for v in (c, b)]
    return ints + [0] * (65 - len(ints)), 0.0, [0, 0, 0, 0, 0]


def _convert(name, a):
    src, sbs, scs, dst, dbs, dcs, to, B, C, P = a[:10]
    return [int(to), B, C, P, _v(sbs), _v(scs), _v(dbs), _v(dcs)], 0.0, [_a(src), _a(dst), 0, 0, 0]


def _masked(name, a):
    src, ss, z, zs, scale, dst, ds, acc, B, C, T, S = a[:12]
    ints = [B, C, T, S, int(acc), int(_v(scale) != 0)] + _arr(ss, 3) + _arr(zs, 3) + _arr(ds, 3)
    return ints, 0.0, [_a(src), _a(z), _a(dst), 0, 0]


def _merge_fwd(name, a):
    B, C, t0, T, up = a[4:9]
    return [B, C, t0, T, up], 0.0, [_a(a[0]), _a(a[1]), _a(a[2]), _a(a[3]), 0]


def _merge_bwd(name, a):
    B, C, t0, T, up = a[6:11]
    return [B, C, t0, T, up, int(_v(a[1]) != 0), int(_v(a[3]) != 0)], 0.0, [_a(a[0]), _a(a[2]), _a(a[4]), _a(a[5]), 0]


DECODE = {n: _pool_fwd for n in ("otal_maxpool3d_fwd", "otal_maxpool3d_fwd_signbits", "otal_maxpool3d_fwd_signbits_h",
                                 "otal_maxpool3d_fwd_io")}
DECODE.update({n: _pool_bwd for n in ("otal_maxpool3d_bwd", "otal_maxpool3d_bwd_signbits", "otal_maxpool3d_bwd_signbits_h",
                                      "otal_maxpool3d_bwd_io")})
DECODE.update({n: _gn_fwd for n in ("otal_gn_relu_fwd", "otal_gn_relu_fwd_to", "otal_gn_relu_fwd_pair", "otal_gn_relu_fwd_pair_to")})
DECODE.update({n: _gn_bwd for n in ("otal_gn_relu_bwd", "otal_gn_relu_bwd_sum", "otal_gn_relu_bwd_pair")})
DECODE.update({"otal_sum_partials": _sum_partials, "otal_convert_storage": _convert, "otal_masked_scale_copy": _masked,
               "otal_pyramid_merge_fwd": _merge_fwd, "otal_pyramid_merge_bwd": _merge_bwd})


class _Recorder:
    """Stands in for the loaded library: the layer entry points are noted, then called."""

    def __init__(self, real):
        self._real = real
        self.calls = []
        self.source = ""

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in DECODE:
            return fn

        def call(*args):
            ints, eps, addr = DECODE[name](name, args)
            ints = [int(v) for v in ints]
            assert len(ints) == len(FIELDS[DECODE[name].__name__[1:]]), (name, len(ints))
            self.calls.append((self.source, name, ints, eps, addr))
            return fn(*args)
        return call


def record(out):
    import torch
    import bench
    from opental_amd import _lib as L
    from opental_amd.common import ops
    rec = _Recorder(L.lib())
    L._lib = rec
    dev = torch.device("cuda", 0)
    ops.CONV_PRECISION = 1              # bf16 MFMA operands: bench.py's default (--dtype bf16)
    for name, batch, half in (("thumos_b8", 8, True), ("thumos_b1", 1, True), ("thumos_b8_fp32", 8, False)):
        saved = ops.HALF_CHAIN, ops.HALF_STORAGE
        ops.HALF_CHAIN = ops.HALF_STORAGE = half
        tr = bench.build_trainer(dev)
        clips, targets, scores = bench.synth_batch(batch, 1000, dev)
        rec.source = name
        tr.step(clips, targets, scores)
        torch.cuda.synchronize()
        ops.STEP.reset()
        del tr
        ops.HALF_CHAIN, ops.HALF_STORAGE = saved
    tr = bench.build_anet_trainer(dev)
    clips, targets, scores = bench.synth_batch(2, 1000, dev, frames=768, classes=150, score_rows=3)
    rec.source = "anet_b2"
    tr.step(clips, targets, scores)
    torch.cuda.synchronize()
    ops.STEP.reset()
    del tr
    from opental_amd.thumos14 import test as T
    from opental_amd.thumos14.BDNet import BDNet
    torch.manual_seed(0)
    net = BDNet(training=False, use_edl=True)
    net.backbone._model.apply(BDNet.weight_init)
    net = net.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    rec.source = "inference"
    T.detect_batch(net, [torch.randint(0, 256, (3, 700, 96, 96), device=dev, generator=g, dtype=torch.uint8)], 10.0, batch_clips=32)
    torch.cuda.synchronize()
    L._lib = rec._real
    c = rec.calls
    cols = dict(source=np.array([r[0] for r in c]), entry=np.array([r[1] for r in c]),
                ints=np.array([r[2] + [0] * (NINTS - len(r[2])) for r in c], np.int64), eps=np.array([r[3] for r in c], np.float32),
                addr16=np.array([r[4] for r in c], np.int64))
    np.savez_compressed(out, **cols)
    # one row per distinct call (the same layer recurs across steps and recipes): the first workload that made it
    seen, keep = set(), []
    for i in range(len(c)):
        key = (str(cols["entry"][i]), tuple(cols["ints"][i].tolist()), float(cols["eps"][i]), tuple(cols["addr16"][i].tolist()))
        if key not in seen:
            seen.add(key)
            keep.append(i)
    np.savez_compressed(GOLDEN, **{k: v[keep] for k, v in cols.items()})
    per = {s: int(np.sum(cols["source"][keep] == s)) for s in dict.fromkeys(cols["source"].tolist())}
    print(f"{len(c)} calls, {len(keep)} distinct -> {GOLDEN}; distinct rows per workload: {per}")


def pool_choice(out):
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import tempfile
    import test_layer_calls_gpu as T
    rows = []
    with T.default_library() as lib, tempfile.TemporaryDirectory() as tmp:
        H = T.PS.build(tmp)
        for item in T.ITEMS:
            label, i, f, _, switches = item
            if not f.startswith("pool"):
                continue
            d, strides, addr, call = T.pool_item(item)
            gen = torch.Generator(device=T.DEV).manual_seed(T.item_seed(item))
            rc, name = T.run_pool(lib, H, label, f, d, strides, addr, call, switches, gen)
            rows.append((label, f, T.pool_ints(d, strides, call), addr, switches, rc, name, -1 if isinstance(i, tuple) else i))
        gen = torch.Generator(device=T.DEV).manual_seed(5)
        for label, f, d, strides, addr, call in T.pool_refusals():
            rc, name = T.run_pool(lib, H, label, f, d, strides, addr, call, (), gen)
            rows.append((label, f, T.pool_ints(d, strides, call), addr, (), rc, name, -1))
    width = len(FIELDS["pool_bwd"])
    np.savez_compressed(out, label=np.array([r[0] for r in rows]), family=np.array([r[1] for r in rows]),
                        ints=np.array([r[2] + [0] * (width - len(r[2])) for r in rows], np.int64),
                        addr16=np.array([r[3] for r in rows], np.int64), switches=np.array([",".join(r[4]) for r in rows]),
                        rc=np.array([r[5] for r in rows], np.int64), kernel=np.array([r[6] for r in rows]),
                        row=np.array([r[7] for r in rows], np.int64))     # row: the item's row of layer_calls.npz, -1 = none
    print(f"{len(rows)} pool items, {len(set(r[6] for r in rows) - {''})} kernels, {sum(r[5] != 0 for r in rows)} refusals -> {out}")


if __name__ == "__main__":
    {"record": record, "pool_choice": pool_choice}[sys.argv[1]](sys.argv[2])

"""CPU: the exact cases of tests/backbone_tape_cases.py hide nothing.  For every case and operand mode: (1) the audit holds -- every
accumulation of the slice stays below 2^24 units, every stored tensor is an fp32 number; (2) torch's fp32 run of the reference is
bit-equal to its float64 run (an independent summation order: what the audit promises, seen once); (3) the case is lively -- no
compared tensor is mostly zero, and the ties a kernel can get wrong are there; (4) it discriminates -- every deliberately wrong
variant of the reference (C.WRONG) changes a compared element wherever the slice has a site for it.  tests/test_backbone_tape_gpu.py
then compares the HIP tape with the same reference without a tolerance."""
import functools

import numpy as np
import pytest
import torch

import backbone_tape_cases as C
from oracle import afsd_oracle as O

LABELS = list(C.SPECS)
MODES = (0, 1)
RUNS = pytest.mark.parametrize("label,mode", C.RUNS, ids=[f"{k}-{m}" for k, m in C.RUNS])


@functools.lru_cache(maxsize=None)
def _ref(label, mode):
    records, live = [], {}
    res = C.reference(C.get_case(label), torch.float64, mode, audit=records, live=live)
    return res, records, live


def test_bf16_rne_is_the_casts_rounding():
    rs = np.random.RandomState(3)
    t = torch.from_numpy(np.concatenate([rs.randn(4096) * 10.0 ** rs.randint(-6, 6, 4096), [0.0, 1.00390625, 1.01171875, -255.5, 3.0]]).astype(np.float32))
    assert torch.equal(C.bf16_rne(t), t.to(torch.bfloat16).float())
    assert torch.equal(C.bf16_rne(t.double()), t.to(torch.bfloat16).double())


def test_window_pool_is_the_oracles_pool():
    """pool_pick (the wrong variant e is its last=True) picks what F.max_pool3d on the zero-padded tensor picks, ties included."""
    rs = np.random.RandomState(4)
    for shape, k, s in (((2, 3, 3, 5, 7), (3, 3, 3), (2, 2, 2)), ((1, 2, 4, 6, 6), (3, 3, 3), (1, 1, 1)), ((1, 2, 2, 6, 8), (1, 3, 3), (1, 2, 2)),
                        ((1, 2, 4, 6, 6), (2, 2, 2), (2, 2, 2))):
        x = torch.from_numpy(rs.randint(-1, 2, shape).astype(np.float64))
        a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = O.maxpool3d_same(a, k, s), C.pool_pick(b, k, s)
        g = torch.from_numpy(rs.randint(1, 5, ya.shape).astype(np.float64))
        ya.backward(g)
        yb.backward(g)
        assert torch.equal(ya, yb) and torch.equal(a.grad, b.grad), (shape, k, s)


@RUNS
def test_audit_holds(label, mode):
    _, records, _ = _ref(label, mode)
    fails, bits = C.audit_failures(records)
    print(f"{label} mode {mode}: the largest accumulation uses {bits:.1f} of {C.MANTISSA} bits")
    assert not fails, fails


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ("only0", "only1", "flat0", "flat1"))
@pytest.mark.parametrize("label", C.HANDOVER_PAIRS)
def test_audit_holds_for_the_other_handover_gradients(label, kind, mode):
    """The GPU file also runs the two-endpoint cases with one gradient zeroed and with one constant over the planes."""
    case = C.get_case(label)
    records = []
    C.reference(case, torch.float64, mode, audit=records, grads=C.handover_grads(case, kind))
    fails, _ = C.audit_failures(records)
    assert not fails, fails


@RUNS
def test_fp32_run_is_bit_equal_to_float64(label, mode):
    want = C.compared(_ref(label, mode)[0])
    got = C.compared(C.reference(C.get_case(label), torch.float32, mode))
    for key, w in want.items():
        assert got[key].dtype == np.float32 and np.array_equal(got[key].astype(np.float64), w), key


@RUNS
def test_case_is_lively(label, mode):
    case = C.get_case(label)
    res, _, live = _ref(label, mode)
    for key, t in C.compared(res).items():
        assert float((t != 0).mean()) >= C.min_nonzero(case, key), (key, float((t != 0).mean()))
    if case.units:
        assert live["pre_zero"] > 0                 # a ReLU input of exactly 0: the mask is (Z > 0), not (Z >= 0)
    if live["pools"]:
        assert live["pool_ties"] > 0                # equal maxima in one window: the first one wins
    if live["padded"] and label not in C.NO_PAD_TIE:
        assert live["pad_ties"] > 0                 # a real 0 against the zero padding


def _sites(case, mode, records):
    """Which wrong variants have a site in this slice (from its structure alone)."""
    kinds = [st[0] for st in case.plan]
    has = {}
    has["a_swap"] = "mixed" in kinds
    has["b_roll"] = "mixed" in kinds or any(k == "conv" for k in kinds[:-1])
    has["c_nomask"] = any(k == "mixed" and kinds[i - 1] != "pool" for i, k in enumerate(kinds) if i > 0)
    has["d_unflip"] = "mixed" in kinds or any(st[0] == "conv" and tuple(st[2]) == C.THREE and (i > 0 or case.need_dx)
                                               for i, st in enumerate(case.plan))
    # a pool whose input carries a gradient: any pool behind a layer; a leading pool or a module's branch pool only with dx
    has["e_last"] = any(k == "pool" and (i > 0 or case.need_dx) for i, k in enumerate(kinds)) or \
        any(k == "mixed" and (i > 0 or case.need_dx) for i, k in enumerate(kinds))
    has["f_rawadd"] = any(st[0] != "pool" for st in case.plan if st[-1] in case.endpoints)
    # g: some gradient operand of a backward GEMM needs more than 8 bits
    has["g_nodz"] = mode == 1 and any(r["kind"] == "conv" and r["g"] is not None and not torch.equal(C.bf16_rne(r["g"]), r["g"])
                                      for r in records)
    return has


@RUNS
def test_wrong_variants_change_a_compared_element(label, mode):
    case = C.get_case(label)
    right = C.compared(_ref(label, mode)[0])
    unrounded = []
    if mode == 1:
        C.reference(case, torch.float64, mode, wrong="g_nodz", audit=unrounded)
    sites = _sites(case, mode, unrounded)
    for wrong in C.WRONG:
        if wrong == "g_nodz" and mode != 1:
            continue
        res = C.reference(case, torch.float64, mode, wrong=wrong)
        if wrong != "g_nodz":
            assert res["applied"] == sites[wrong], (wrong, "site", res["applied"], sites[wrong])
        if not sites[wrong]:
            continue
        got = C.compared(res)
        changed = [k for k in right if not np.array_equal(right[k], got[k])]
        assert changed, f"{label} mode {mode}: '{C.WRONG[wrong]}' goes unseen"


def test_every_wrong_variant_has_a_site_somewhere():
    seen = set()
    for label in C.FP32_STORED:
        case = C.get_case(label)
        seen |= {w for w, on in _sites(case, 0, []).items() if on}
    assert seen | {"g_nodz"} == set(C.WRONG)

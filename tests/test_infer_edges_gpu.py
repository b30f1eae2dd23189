"""GPU: the inference post-processing kernels (csrc/infer.hip) at their edges, through the C ABI, against the float64 references of
tests/infer_cases.py (tests/test_infer_cases_cpu.py proves the references and the cases' structure on the CPU).

Soft-NMS (otal_softnms_classes_ws): every output starts as a sentinel bit pattern between guards.  Per (video, class) problem the
kept index set, the count and out_index equal the reference exactly, with no case and no row left out; start / end / unct / actn are
copies and compared bit for bit; the score bit for bit where it cannot change (disjoint segments: ties, threshold equality, layout,
isolation, the LDS / scratch boundary) and within NMS_SAFETY * NMS_UNITS * rounds * 2^-24 relative where it decays; rows and
index entries at and past the count keep the sentinel, so a problem cannot have touched its neighbours.  Decode (otal_decode_clips,
_ex, _ev): seg, score, unct, actn within the tolerances of tests/test_infer_gpu.py (score / unct rtol max(1e-5, 2 K 2^-24)), flags
exact wherever infer_cases.flags_compared says a float32 decode must reproduce them, the three entries bit-identical where they
overlap, NULL unct / actn without effect on the rest.  Refused calls return their code and write nothing.

`pytest -s` prints the largest observed deviation per family against its tolerance at the end of the run.  Measured on an MI355X,
as a fraction of the tolerance: Soft-NMS decayed scores 0.0019 (random, 7.6e-07 of rtol 4.0e-04 after 106 rounds), 0.0011
(duplicates), 0.0007 (degenerate); decode seg <= 0.090, score <= 0.076, unct <= 0.068, actn <= 0.013 over the 35 cases.

What each fault would trip (argued from csrc/infer.hip; tests/test_infer_cases_cpu.py models the first two in numpy):
  `>=` in the in-thread scan       a thread keeps the LAST maximum of its stride: ties-top1 keeps a later row instead of row 69;
  best_merge preferring the higher index   lanes / waves hand up a later row: ties-top1 .. top257 and all_equal keep other rows;
  lds_cap one short                the 7680th row of boundary_rows[7680] and of video 0 of boundary_batch -- the best score -- is
                                   dropped by `p < cap`, the kept set changes; without that guard ts[7679] aliases te[0] and row 0,
                                   which is kept, comes out with another end (compared bit for bit);
  a one-pass decode loop           anchors 128 .. A - 1 of the A = 129 / 189 / 300 cases keep the sentinel: "elements left unwritten";
  a (video, class) problem writing past its count, or into a neighbour: the sentinel checks of check_nms and the guards."""
import ctypes

import numpy as np
import pytest
import torch

import infer_cases as IC

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -7
GUARD = 64
SENT32, SENT8 = 0x7F7FBEEF, 0xA5        # a finite float / an index and a count no case produces; flags are 0 or 1
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from opental_amd import _lib as L
    lb = L.lib()
    yield lb
    if WORST:
        print("\nlargest observed deviation / tolerance per family:")
        for k in sorted(WORST):
            print(f"  {k:28s} {WORST[k][0]:.4f}   ({WORST[k][1]})")


def worst(family, ratio, what):
    if ratio > WORST.get(family, (-1.0, ""))[0]:
        WORST[family] = (float(ratio), what)


def stream():
    from opental_amd import _lib as L
    return L.stream()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Out:
    """A device buffer of `shape` (int32-sized elements, or bytes) filled with sentinel bits, with GUARD elements in front and
    behind."""

    def __init__(self, shape, byte=False):
        self.n = int(np.prod(shape))
        self.shape, self.sent = tuple(shape), SENT8 if byte else SENT32
        self.base = torch.full((self.n + 2 * GUARD,), self.sent, dtype=torch.uint8 if byte else torch.int32, device="cuda")
        self.p = ctypes.c_void_p(self.base.data_ptr() + GUARD * self.base.element_size())

    def bits(self, label):
        """The buffer's elements as a numpy integer array of `shape`; the guards must hold the sentinel."""
        a = self.base.cpu().numpy()
        assert (a[:GUARD] == self.sent).all() and (a[GUARD + self.n:] == self.sent).all(), f"{label}: a guard element changed"
        return a[GUARD:GUARD + self.n].reshape(self.shape)

    def untouched(self, label):
        return bool((self.bits(label) == self.sent).all())


def f32(bits):
    return np.ascontiguousarray(bits).view(np.float32)


def i32(values):
    return np.ascontiguousarray(values, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ Soft-NMS
def run_nms(lib, batch, sigma, top_k, thr, out_cols=5, index=True, unct=True, actn=True):
    d = {k: dev(batch[k]) for k in ("seg", "score", "unct", "actn", "flag")}
    cs = torch.tensor(batch["clip_start"], dtype=torch.int32).cuda()
    V, K, A = len(batch["clip_start"]) - 1, batch["K"], batch["A"]
    max_clips, total = int(np.diff(batch["clip_start"]).max()), int(batch["clip_start"][-1])
    out, counts, idx = Out((V, K, top_k, max(out_cols, 1))), Out((V, K)), Out((V, K, top_k))
    nbytes = int(lib.otal_softnms_scratch_bytes(total, max_clips, A, K))
    assert (nbytes > 0) == (max_clips * A > IC.LDS_ROWS)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    rc = lib.otal_softnms_classes_ws(ptr(d["seg"]), ptr(d["score"]), ptr(d["unct"] if unct else None),
                                     ptr(d["actn"] if actn else None), ptr(d["flag"]), ptr(cs), V, max_clips, A, K,
                                     sigma, top_k, thr, out.p, counts.p, idx.p if index else None,
                                     out_cols, ptr(scratch), nbytes, total, stream())
    torch.cuda.synchronize()
    return rc, out, counts, idx


def check_nms(name, out, counts, idx, cols=5, fill=SENT32):
    """out (V, K, top_k, cols) / counts (V, K) / idx (V, K, top_k) or None as int32 bit arrays, against the references of the case."""
    c = IC.nms_case(name)
    for (v, k), (rows, src, ref) in IC.nms_references(name).items():
        kept = np.nonzero(ref["kept"])[0]
        cnt = int(counts[v, k])
        assert cnt == len(kept), (name, v, k, cnt, len(kept))
        got = out[v, k, :cnt]
        want = i32(rows[kept])
        for col in (0, 1) + tuple(range(3, cols)):                          # copies: bit for bit
            assert np.array_equal(got[:, col], want[:, col]), (name, v, k, col)
        if c["exact"]:
            assert np.array_equal(got[:, 2], want[:, 2]), (name, v, k)
        elif cnt:
            tol = IC.NMS_SAFETY * IC.nms_bound(ref["rounds"])
            dev_ = np.abs(f32(got[:, 2]).astype(np.float64) - ref["score"][kept]) / ref["score"][kept]
            worst("softnms " + name.split("-")[0], dev_.max() / tol, f"{name}: {dev_.max():.3e} of rtol {tol:.3e}, {ref['rounds']} rounds")
            assert dev_.max() <= tol, (name, v, k, dev_.max(), tol)
        assert (out[v, k, cnt:] == fill).all(), (name, v, k, "rows at and past the count were written")
        if idx is not None:
            assert np.array_equal(idx[v, k, :cnt], src[kept]), (name, v, k)
            assert (idx[v, k, cnt:] == fill).all(), (name, v, k, "index entries at and past the count were written")


@pytest.mark.parametrize("name", list(IC.NMS_CASES))
def test_softnms_case(lib, name):
    c = IC.nms_case(name)
    rc, out, counts, idx = run_nms(lib, c["batch"], c["sigma"], c["top_k"], c["thr"])
    assert rc == 0
    check_nms(name, out.bits("out"), counts.bits("counts"), idx.bits("index"))


def test_boundary_batch_through_softnms_classes():
    """One video exactly at the LDS working set, one past it (scratch), one without clips and a short one, as the drivers launch
    them (common.detect.softnms_classes: outputs zero-filled)."""
    from opental_amd.common.detect import softnms_classes
    c = IC.nms_case("boundary_batch")
    dec = {k: dev(c["batch"][k]) for k in ("seg", "score", "unct", "actn", "flag")}
    rows, counts, index = softnms_classes(dec, c["batch"]["clip_start"], top_k=c["top_k"], sigma=c["sigma"], score_threshold=float(c["thr"]))
    assert rows.shape == (4, 2, 64, 5) and index.shape == (4, 2, 64)
    check_nms("boundary_batch", i32(rows.cpu().numpy()), counts.cpu().numpy(), index.cpu().numpy(), fill=0)


@pytest.mark.parametrize("n", IC.BOUNDARY_ROWS)
def test_boundary_rows_through_softnms_v2(n):
    """7680 candidates fill the LDS working set to its last row, 7681 run from the scratch; the two best rows are the last two."""
    from opental_amd.common.segment_utils import softnms_v2
    rows, ref = IC.boundary_rows(n)
    got, cnt, mask = softnms_v2(dev(rows), sigma=0.5, top_k=IC.BOUNDARY_TOP_K, score_threshold=float(IC.THR), use_edl=True,
                                os_head=True, get_mask=True)
    assert int(cnt) == IC.BOUNDARY_TOP_K and np.array_equal(mask.cpu().numpy(), ref["kept"])
    assert np.array_equal(i32(got.cpu().numpy()), i32(rows[ref["kept"]]))               # disjoint segments: every column is a copy


def test_top_k_zero_keeps_nothing():
    """softnms_v2(top_k=0): the reference's loop (`done.sum() < top_k`) never runs."""
    from opental_amd.common.segment_utils import softnms_v2
    rows = IC.nms_case("random-n64-s0.5-top20")["batch"]
    x = np.concatenate([rows["seg"][0], rows["score"][0, 0][:, None], rows["unct"][0][:, None], rows["actn"][0][:, None]], 1)
    assert not IC.softnms_reference(x, 0.5, 0, IC.THR)["kept"].any()
    got, cnt, mask = softnms_v2(dev(x), sigma=0.5, top_k=0, use_edl=True, os_head=True, get_mask=True)
    assert tuple(got.shape) == (0, 5) and int(cnt) == 0 and mask.shape == (64,) and not bool(mask.any())
    got, cnt = softnms_v2(dev(x)[:, :3].contiguous(), sigma=0.5, top_k=0)
    assert tuple(got.shape) == (0, 3) and int(cnt) == 0


@pytest.mark.parametrize("A", list(IC.LAYOUT))
def test_narrow_rows_equal_the_leading_columns(lib, A):
    """out_cols 3 / 4 with NULL unct / actn and NULL out_index: the leading columns of the 5-column run, bit for bit."""
    name = f"layout-A{A}"
    c = IC.nms_case(name)
    b = c["batch"]
    top_k = int(np.diff(b["clip_start"]).max()) * A
    rc, out5, counts5, idx5 = run_nms(lib, b, c["sigma"], top_k, c["thr"])
    assert rc == 0
    full, cnt = out5.bits("out"), counts5.bits("counts")
    check_nms(name, full, cnt, idx5.bits("index"))
    for cols in (3, 4):
        rc, out, counts, idx = run_nms(lib, b, c["sigma"], top_k, c["thr"], out_cols=cols, index=False, unct=cols > 3, actn=False)
        assert rc == 0 and idx.untouched("index")
        assert np.array_equal(counts.bits("counts"), cnt) and np.array_equal(out.bits("out"), full[..., :cols])
        check_nms(name, out.bits("out"), cnt, None, cols=cols)


def test_refused_softnms_arguments_write_nothing(lib):
    c = IC.nms_case("layout-A5")
    for kw, code in ((dict(out_cols=2), E_SHAPE), (dict(out_cols=6), E_SHAPE), (dict(out_cols=5, actn=False), E_NULL),
                     (dict(out_cols=4, unct=False), E_NULL)):
        rc, out, counts, idx = run_nms(lib, c["batch"], c["sigma"], 8, c["thr"], **kw)
        assert rc == code, (kw, rc)
        assert out.untouched("out") and counts.untouched("counts") and idx.untouched("index"), kw
    rc, out, counts, idx = run_nms(lib, c["batch"], c["sigma"], 0, c["thr"])                # top_k 0: nothing to keep, no launch
    assert rc == E_SHAPE and counts.untouched("counts")


# ------------------------------------------------------------------------------------------------ decode
DECODE_OUT = ("seg", "score", "unct", "actn", "flag")


def run_decode(lib, case, entry, unct=True, actn=True, **override):
    """entry: 'plain' (otal_decode_clips), 'ex' or 'ev'.  override: n / K / score_fn / first_class / evidence / act / prop_act as
    passed to the call (the buffers keep the case's sizes).  -> (return code, {name: Out})."""
    ins = case["inputs"]
    n, A, K = case["shape"]
    KO = K - case["first_class"]
    d = {k: dev(v) for k, v in ins.items()}
    outs = dict(seg=Out((n, A, 2)), score=Out((n, KO, A)), unct=Out((n, A)), actn=Out((n, A)), flag=Out((n, KO, A), byte=True))
    act = override.get("act", d.get("act"))
    prop_act = override.get("prop_act", d.get("prop_act"))
    args = [ptr(d["loc"]), ptr(d["prop_loc"]), ptr(d["priors"]), ptr(d["conf"]), ptr(d["prop_conf"]), ptr(d["center"]), ptr(act),
            ptr(prop_act), ptr(d["offsets"]), ptr(d["fps"]), outs["seg"].p, outs["score"].p, outs["unct"].p if unct else None,
            outs["actn"].p if actn else None, outs["flag"].p, n, A, override.get("K", K), case["clip_length"],
            case["conf_thresh"]]
    fn = [override.get("score_fn", case["score_fn"]), override.get("first_class", case["first_class"])]
    if entry == "plain":
        rc = lib.otal_decode_clips(*args, stream())
    elif entry == "ex":
        rc = lib.otal_decode_clips_ex(*args, *fn, stream())
    else:
        rc = lib.otal_decode_clips_ev(*args, *fn, override.get("evidence", case["evidence"]), stream())
    torch.cuda.synchronize()
    return rc, outs


def _bits(outs, skip=()):
    return {k: outs[k].bits(k) for k in DECODE_OUT if k not in skip}


def _ratio(got, ref, rtol, atol):
    return float((np.abs(got.astype(np.float64) - ref) / (atol + rtol * np.abs(ref))).max())


@pytest.mark.parametrize("name", IC.DECODE_CASES)
def test_decode_case(lib, name):
    case, ref = IC.decode_case(name), IC.decode_ref(name)
    n, A, K = case["shape"]
    cfg = name.split("-")[0]
    rc, outs = run_decode(lib, case, "ev")
    assert rc == 0
    b = _bits(outs)
    for k in ("seg", "score", "unct", "actn"):
        assert not (b[k] == SENT32).any(), f"{k}: elements left unwritten"
    assert np.isin(b["flag"], (0, 1)).all()
    rt = IC.score_rtol(K)
    for k, (rtol, atol) in (("seg", IC.SEG_TOL), ("score", (rt, IC.SCORE_ATOL)), ("unct", (rt, IC.SCORE_ATOL)), ("actn", IC.ACTN_TOL)):
        r = _ratio(f32(b[k]), ref[k], rtol, atol)
        print(f"{name} {k}: largest deviation {r:.4f} of its tolerance (rtol {rtol:.3g}, atol {atol:.3g})")
        worst(f"decode {cfg} {k}", r, name)
        np.testing.assert_allclose(f32(b[k]), ref[k], rtol=rtol, atol=atol, err_msg=f"{name} {k}")
    cmp = IC.flags_compared(ref, K, case["planted_an"])
    assert np.array_equal(b["flag"][cmp].astype(bool), ref["flag"][cmp]), name
    if case["has_act"]:
        pl = case["planted_an"]
        assert (f32(b["actn"])[pl] == 0.5).all() and not b["flag"].transpose(0, 2, 1)[pl].any()      # an == 0.5 exactly: never flagged
    # the entries agree bit for bit where they overlap
    if case["evidence"] == IC.EXP:
        rc, ex = run_decode(lib, case, "ex")
        assert rc == 0 and all(np.array_equal(v, b[k]) for k, v in _bits(ex).items())
    if cfg == "opental_exp":
        rc, plain = run_decode(lib, case, "plain")
        assert rc == 0 and all(np.array_equal(v, b[k]) for k, v in _bits(plain).items())
    # NULL unct / actn: not written, the rest unchanged
    rc, part = run_decode(lib, case, "ev", unct=False, actn=False)
    assert rc == 0 and part["unct"].untouched("unct") and part["actn"].untouched("actn")
    assert all(np.array_equal(v, b[k]) for k, v in _bits(part, skip=("unct", "actn")).items())


def test_refused_decode_arguments_write_nothing(lib):
    closed, os_ = IC.decode_case("closed_exp-2x1x2"), IC.decode_case("opental_exp-3x128x15")
    act = dev(os_["inputs"]["act"])
    calls = [(closed, "ex", dict(K=1), E_SHAPE),                                # K - first_class <= 0
             (closed, "ev", dict(K=1), E_SHAPE),
             (closed, "ex", dict(score_fn=2), E_UNSUPPORTED),
             (closed, "ev", dict(score_fn=2), E_UNSUPPORTED),
             (closed, "ev", dict(evidence=3), E_UNSUPPORTED),
             (os_, "ev", dict(evidence=-1), E_UNSUPPORTED),
             (os_, "ex", dict(act=None), E_NULL),                               # one of act / prop_act NULL
             (os_, "ev", dict(prop_act=None), E_NULL),
             (closed, "ex", dict(act=act), E_NULL),
             (os_, "plain", dict(act=None, prop_act=None), E_NULL)]             # the OpenTAL entry needs every map
    for case, entry, kw, code in calls:
        rc, outs = run_decode(lib, case, entry, **kw)
        assert rc == code, (entry, kw, rc)
        assert all(outs[k].untouched(k) for k in DECODE_OUT), (entry, kw)
    rc, outs = run_decode(lib, os_, "plain", unct=False)
    assert rc == E_NULL and all(outs[k].untouched(k) for k in DECODE_OUT)

"""CPU: the references and cases of tests/infer_cases.py, so that tests/test_infer_edges_gpu.py hides nothing.

softnms_reference and decode_reference (float64) reproduce the reference-generated fixtures (tests/golden/softnms.npz,
decode_b2.npz, closed_set.npz, evidence.npz) within the tolerances the GPU tests of those fixtures use; on every Soft-NMS case the
float64 reference, the fp32 torch restatement and the fp32 C restatement of the oracle keep the same rows; every random case meets
its decision margin; every decode case leaves fewer than FLAG_SKIP_CAP of its flags uncompared; and the exact cases have the
structure they claim (disjoint segments, ties in the three thread positions, 7680 / 7681 rows, anchors on every clamp)."""
import os

import numpy as np
import pytest
import torch

import ablations_common as AC
import evidence_common as E
import infer_cases as IC
from oracle import afsd_oracle as O

NMS_THREADS = 256           # csrc/infer.hip: threads of a Soft-NMS workgroup, four waves of 64


# ------------------------------------------------------------------------------------------------ Soft-NMS
def test_softnms_reference_reproduces_the_golden_vectors(golden_dir):
    fx = np.load(os.path.join(golden_dir, "softnms.npz"))
    runs = [(n, 5000, f"mask_{n}", f"rows_{n}") for n in (0, 1, 2, 50, 400, 2000)] + [(400, 20, "mask_400_top20", "rows_400_top20")]
    for n, top_k, mask, rows in runs:
        x = fx[f"in_{n}"]
        ref = IC.softnms_reference(x, 0.5, top_k, 0.001)
        assert np.array_equal(ref["kept"], fx[mask]), (n, top_k)
        got = np.concatenate([x[ref["kept"], :2], ref["score"][ref["kept"], None], x[ref["kept"], 3:]], 1)
        np.testing.assert_allclose(got, fx[rows], rtol=2e-6, atol=1e-7)


def _oracles_agree(rows, ref, sigma, top_k, thr):
    if len(rows) == 0:
        assert ref["kept"].size == 0
        return
    t = torch.from_numpy(rows)
    _, c_t, m_t = O.softnms_v2(t, sigma=float(sigma), top_k=top_k, score_threshold=float(thr))
    _, c_c, m_c = O.softnms_v2_c(t, sigma=float(sigma), top_k=top_k, score_threshold=float(thr))
    assert np.array_equal(ref["kept"], m_t.numpy()) and c_t == int(ref["kept"].sum())
    assert np.array_equal(ref["kept"], m_c.numpy()) and c_c == int(ref["kept"].sum())


@pytest.mark.parametrize("name", list(IC.NMS_CASES))
def test_float64_torch_and_c_references_keep_the_same_rows(name):
    c = IC.nms_case(name)
    for (v, k), (rows, src, ref) in IC.nms_references(name).items():
        assert np.isfinite(ref["score"]).all(), (v, k)
        _oracles_agree(rows, ref, c["sigma"], c["top_k"], c["thr"])


@pytest.mark.parametrize("name", list(IC.NMS_CASES))
def test_exact_cases_are_disjoint_with_unchanged_scores(name):
    c = IC.nms_case(name)
    if not c["exact"]:
        return
    for (v, k), (rows, src, ref) in IC.nms_references(name).items():
        assert IC.is_disjoint(rows), (v, k)
        assert np.array_equal(ref["score"], rows[:, 2].astype(np.float64)), (v, k)


@pytest.mark.parametrize("name", IC.MARGIN_CASES)
def test_inexact_cases_meet_their_decision_margin(name):
    rows, src, ref = IC.nms_references(name)[(0, 0)]
    bound = IC.nms_bound(ref["rounds"])
    print(f"{name}: rounds {ref['rounds']}, margin {ref['margin']:.3e}, bound {bound:.3e}, kept {int(ref['kept'].sum())}")
    assert ref["margin"] >= IC.NMS_SAFETY * bound
    decayed = ref["score"] < rows[:, 2]
    assert ref["rounds"] > 1 and decayed.any()
    if name.startswith("random-"):
        assert (decayed & ref["kept"]).sum() >= 10                                  # rows are taken after their scores decayed


def test_random_cases_cover_every_size_sigma_and_top_k():
    assert {(n, s) for n in (64, 150, 300) for s in (0.5, 0.85)} == set(IC.RANDOM_SEEDS)
    assert len(IC.RANDOM_CASES) == 12
    for name in IC.RANDOM_CASES:
        ref = IC.nms_references(name)[(0, 0)][2]
        if name.endswith("top20"):
            assert ref["rounds"] == 20 and int(ref["kept"].sum()) == 20             # the truncation is what ends the loop


def test_ties_sit_in_the_three_thread_positions():
    rows = IC.nms_case("ties-top1")["batch"]
    sc = rows["score"].reshape(-1)
    assert len(sc) == 1000 and set(np.unique(sc).tolist()) == set(np.asarray(IC.TIE_VALUES, np.float32).tolist())
    top = np.nonzero(sc == sc.max())[0]
    first = int(top[0])
    assert first == IC.TIE_FIRST
    tid, lane_wave = top % NMS_THREADS, (top % NMS_THREADS) // 64
    assert ((tid == first % NMS_THREADS) & (top > first)).sum() >= 2                # same thread: i + 256, i + 512
    assert ((lane_wave == first // 64) & (tid != first) & (top < NMS_THREADS)).any()    # another lane of the same wave
    assert set(lane_wave.tolist()) == {0, 1, 2, 3}         # every wave holds one (wave 0 from a later sweep: the first is in wave 1)
    for value in IC.TIE_VALUES:                                                     # every value ties across all three
        idx = np.nonzero(sc == np.float32(value))[0]
        assert len(idx) > 100 and len(set((idx % NMS_THREADS).tolist())) < len(idx)
    order = np.lexsort((np.arange(1000), -sc.astype(np.float64)))                   # score descending, index ascending
    for top_k in IC.TIE_TOP_K:
        ref = IC.nms_references(f"ties-top{top_k}")[(0, 0)][2]
        want = np.zeros(1000, bool)
        want[order[:min(top_k, 999)]] = True                                        # the last survivor is never kept
        assert np.array_equal(ref["kept"], want), top_k


def _kernel_pick(sc, undone, strict=True, prefer="low"):
    """The kernel's maximum among undone as a numpy model of its three levels (csrc/infer.hip, the greedy loop): each of 256
    threads scans i = tid, tid + 256, ... with `>` (strict) or `>=`; the 64 lanes of a wave merge by the __shfl_down tree of
    best_merge; the four waves merge in order.  prefer: which index best_merge takes among equal scores ('low' is the kernel)."""
    def merge(a, b):
        if b[1] < 0:
            return a
        if a[1] < 0 or b[0] > a[0] or (b[0] == a[0] and (b[1] < a[1] if prefer == "low" else b[1] > a[1])):
            return b
        return a
    best = []
    for tid in range(NMS_THREADS):
        b = (0.0, -1)
        for i in range(tid, len(sc), NMS_THREADS):
            if undone[i] and (b[1] < 0 or (sc[i] > b[0] if strict else sc[i] >= b[0])):
                b = (sc[i], i)
        best.append(b)
    waves = []
    for w in range(NMS_THREADS // 64):
        lanes = best[64 * w:64 * w + 64]
        o = 32
        while o:
            lanes = [merge(lanes[l], lanes[l + o]) if l + o < 64 else lanes[l] for l in range(64)]
            o >>= 1
        waves.append(lanes[0])
    b = waves[0]
    for w in waves[1:]:
        b = merge(b, w)
    return b[1]


@pytest.mark.parametrize("top_k", [1, 7, 255])
def test_tie_cases_tell_the_kernels_tie_break_from_its_neighbours(top_k):
    """On disjoint segments Soft-NMS is top_k picks.  The model of the kernel's pick equals the reference; with `>=` in the
    in-thread scan, or with best_merge preferring the higher index, the kept set differs already at top_k = 1."""
    sc = IC.nms_case("ties-top1")["batch"]["score"].reshape(-1)
    want = IC.nms_references(f"ties-top{top_k}")[(0, 0)][2]["kept"]
    for kw, same in ((dict(), True), (dict(strict=False), False), (dict(prefer="high"), False)):
        undone, kept = np.ones(len(sc), bool), np.zeros(len(sc), bool)
        for _ in range(top_k):
            j = _kernel_pick(sc, undone, **kw)
            undone[j], kept[j] = False, True
        assert np.array_equal(kept, want) == same, kw


def test_all_equal_and_threshold_equality_keep_what_they_claim():
    ref = IC.nms_references("all_equal")[(0, 0)][2]
    assert ref["kept"].size == 513 and np.array_equal(np.nonzero(ref["kept"])[0], np.arange(100))
    rows, _, ref = IC.nms_references("thr_equality")[(0, 0)]
    sc = rows[:, 2]
    at, below = np.nonzero(sc == IC.THR)[0], np.nonzero(sc == np.nextafter(IC.THR, np.float32(0)))[0]
    assert len(at) == 15 and len(below) == 15 and (sc[below] < IC.THR).all()
    want = np.zeros(len(sc), bool)
    want[sc > IC.THR] = True
    want[at[:-1]] = True                # equal to thr: candidates, taken in index order; the last survivor is never kept
    assert np.array_equal(ref["kept"], want) and not ref["kept"][below].any()


@pytest.mark.parametrize("sigma", [0.5, 0.85])
def test_duplicates_have_iou_one_and_decays_far_from_the_threshold(sigma):
    rows, _, ref = IC.nms_references(f"duplicates-s{sigma}")[(0, 0)]
    starts, counts = np.unique(rows[:, 0], return_counts=True)
    assert len(starts) == 14 and (counts == 3).all() and (rows[:, 1] - rows[:, 0] == 4.0).all()
    assert ref["margin"] > 0.01                                                     # >= 500 x the bound of its rounds
    decayed = ref["score"] < rows[:, 2]
    assert (decayed & (ref["score"] < IC.DUP_THR)).any()                            # one decay drops some members ...
    if sigma == 0.85:
        assert (decayed & ref["kept"]).any()                                        # ... and leaves others to be kept


def test_degenerate_case_mixes_zero_width_and_reversed_segments():
    rows, _, ref = IC.nms_references("degenerate")[(0, 0)]
    w = rows[:, 1] - rows[:, 0]
    assert (w == 0).sum() == 8 and (w < 0).sum() == 8 and (w > 0).sum() == 48
    assert np.abs(w[w < 0]).min() >= 0.25                      # width + (end - start) is never 0: no 0 / 0
    assert ref["kept"][w <= 0].any() and ref["kept"][w > 0].any()


@pytest.mark.parametrize("n", IC.BOUNDARY_ROWS)
def test_boundary_rows_need_the_whole_working_set(n):
    rows, ref = IC.boundary_rows(n)
    assert rows.shape[0] == n and IC.is_disjoint(rows) and len(np.unique(rows[:, 2])) == n
    assert int(ref["kept"].sum()) == IC.BOUNDARY_TOP_K and ref["kept"][[0, n - 2, n - 1]].all()
    order = np.argsort(-rows[:, 2].astype(np.float64))
    assert set(order[:IC.BOUNDARY_TOP_K].tolist()) == set(np.nonzero(ref["kept"])[0].tolist())
    short = IC.softnms_reference(rows[:-1], 0.5, IC.BOUNDARY_TOP_K, IC.THR)         # a working set one row short
    assert not np.array_equal(np.nonzero(short["kept"])[0], np.nonzero(ref["kept"])[0])
    _oracles_agree(rows, ref, 0.5, IC.BOUNDARY_TOP_K, IC.THR)


def test_boundary_batch_has_one_video_on_each_side_of_the_working_set():
    refs = IC.nms_references("boundary_batch")
    b = IC.nms_case("boundary_batch")["batch"]
    assert b["A"] == 128 and b["K"] == 2
    assert [len(refs[(v, 0)][0]) for v in range(4)] == [IC.LDS_ROWS, IC.LDS_ROWS + 128, 0, 128]
    assert [int(refs[(v, 1)][2]["kept"].sum()) for v in range(4)] == [64, 64, 0, 64]


@pytest.mark.parametrize("A", list(IC.LAYOUT))
def test_layout_cases_straddle_clips_and_have_empty_parts(A):
    c = IC.nms_case(f"layout-A{A}")
    b = c["batch"]
    clips = np.diff(b["clip_start"])
    assert b["K"] == 3 and b["flag"][:, 1].sum() == 0 and (clips * A).max() > NMS_THREADS
    assert all(b["flag"][i].sum() == 0 for i in IC.LAYOUT_EMPTY_CLIPS[A])
    if A < NMS_THREADS // 2:
        assert NMS_THREADS // A + 1 >= 3                       # a chunk of 256 rows holds rows of at least three clips
    counts = [len(rows) for rows, _, _ in IC.nms_references(f"layout-A{A}").values()]
    assert max(counts) > NMS_THREADS // 4 and 0 in counts
    iso = [(len(rows), int(ref["kept"].sum())) for rows, _, ref in IC.nms_references(f"isolation-A{A}").values()]
    assert any(n > 6 and k == 5 for n, k in iso)               # problems that top_k = 5 truncates ...
    assert any(k < 5 for n, k in iso)                          # ... next to problems with fewer rows to keep


# ------------------------------------------------------------------------------------------------ decode
def _check_decode(ref, want_seg, want_score, want_unct, want_actn, want_mask, K, ci):
    np.testing.assert_allclose(ref["seg"][ci], want_seg, rtol=IC.SEG_TOL[0], atol=IC.SEG_TOL[1])
    np.testing.assert_allclose(ref["score"][ci], want_score, rtol=IC.score_rtol(K), atol=IC.SCORE_ATOL)
    if want_unct is not None:
        np.testing.assert_allclose(ref["unct"][ci], want_unct, rtol=IC.score_rtol(K), atol=IC.SCORE_ATOL)
    if want_actn is not None:
        np.testing.assert_allclose(ref["actn"][ci], want_actn, rtol=IC.ACTN_TOL[0], atol=IC.ACTN_TOL[1])
    cmp = IC.flags_compared(ref, K)[ci]
    assert cmp.mean() > 1 - IC.FLAG_SKIP_CAP
    assert np.array_equal(ref["flag"][ci][cmp], want_mask.astype(bool)[cmp])


def test_decode_reference_reproduces_the_opental_fixture(golden_dir):
    fx, want = np.load(os.path.join(golden_dir, "thumos_b2.npz")), np.load(os.path.join(golden_dir, "decode_b2.npz"))
    ins = {k: fx["out_" + k] for k in ("loc", "conf", "prop_loc", "prop_conf", "center", "act", "prop_act")}
    ins.update(priors=O.priors_all().numpy(), offsets=np.float32([0.0, 384.0]), fps=np.float32([10.0, 10.0]))
    ref = IC.decode_reference(ins, 256, 0.01, 0, 0, IC.EXP, True)
    for ci in (0, 1):
        mask = (want[f"score_{ci}"] > 0.01) & (want[f"act_{ci}"] > 0.5)
        _check_decode(ref, want[f"seg_{ci}"], want[f"score_{ci}"], want[f"unct_{ci}"], want[f"act_{ci}"], mask, 15, ci)


@pytest.mark.parametrize("use_edl", [False, True])
@pytest.mark.parametrize("fusion", [False, True])
def test_decode_reference_reproduces_the_closed_set_fixture(golden_dir, use_edl, fusion):
    fx = np.load(os.path.join(golden_dir, "closed_set.npz"))
    ins = AC.head_outputs(31, 16, False, B=2)           # the draws of tools/pin_closed_set.py
    if fusion:                                          # both clips decode the fp32 average of the two samples
        ins = {k: np.broadcast_to(((v[0] + v[1]) / np.float32(2.0))[None], v.shape).copy() for k, v in ins.items()}
    ins.update(priors=AC.priors().numpy(), offsets=np.float32(fx["clips"][:, 0]), fps=np.float32(fx["clips"][:, 1]))
    ref = IC.decode_reference(ins, 256, 0.01, 0 if use_edl else 1, 1, IC.EXP, False)
    tag = f"dec_edl{int(use_edl)}_fus{int(fusion)}"
    for ci in (0, 1):
        unct = fx[f"{tag}_unct_{ci}"] if use_edl and not fusion else None       # a fused run reports the networks' own maps
        _check_decode(ref, fx[f"{tag}_seg_{ci}"], fx[f"{tag}_score_{ci}"][1:], unct, None, fx[f"{tag}_mask_{ci}"][1:], 16, ci)


@pytest.mark.parametrize("os_head", [True, False])
@pytest.mark.parametrize("kind", ["relu", "softplus"])
def test_decode_reference_reproduces_the_evidence_fixture(golden_dir, kind, os_head):
    fx = np.load(os.path.join(golden_dir, "evidence.npz"))
    K = 15 if os_head else 16
    ins = E.head_outputs(int(fx["seed"]), K, os_head)
    ins.update(priors=AC.priors().numpy(), offsets=np.float32([c[0] for c in E.CLIPS]), fps=np.float32([c[1] for c in E.CLIPS]))
    ref = IC.decode_reference(ins, 256, E.CONF_THRESH, 0, 0 if os_head else 1, E.EVIDENCE.index(kind), os_head)
    tag = f"dec_{kind}_{'os' if os_head else 'closed'}"
    for ci in (0, 1):
        _check_decode(ref, fx[f"{tag}_seg_{ci}"], fx[f"{tag}_score_{ci}"], fx[f"{tag}_unct_{ci}"],
                      fx[f"{tag}_actn_{ci}"] if os_head else None, fx[f"{tag}_mask_{ci}"], K, ci)


def test_decode_cases_cover_every_configuration_and_shape():
    assert len(IC.DECODE_CASES) == 35 and len(set(IC.DECODE_CASES)) == 35
    for cfg, (score_fn, first_class, evidence, has_act) in IC.CONFIGS.items():
        shapes = {IC.decode_case(n)["shape"] for n in IC.DECODE_CASES if n.startswith(cfg + "-")}
        assert shapes == set(IC.SHAPES[first_class]) and has_act == (first_class == 0)
    assert set(IC.OFFSETS) == {float(o) for n in IC.DECODE_CASES for o in IC.decode_case(n)["inputs"]["offsets"]}
    assert {np.float32(f) for f in IC.FPS} == {f for n in IC.DECODE_CASES for f in IC.decode_case(n)["inputs"]["fps"]}


@pytest.mark.parametrize("name", IC.DECODE_CASES)
def test_decode_case_keeps_its_flags_and_sits_on_its_edges(name):
    c, ref = IC.decode_case(name), IC.decode_ref(name)
    n, A, K = c["shape"]
    N = n * A
    for k in ("seg", "score", "unct", "actn"):
        assert np.isfinite(ref[k]).all(), k
    cmp = IC.flags_compared(ref, K, c["planted_an"])
    skipped = 1.0 - cmp.mean()
    print(f"{name}: {cmp.size - int(cmp.sum())} of {cmp.size} flags left out ({100 * skipped:.4f} %), flagged {ref['flag'].mean():.3f}")
    assert skipped < IC.FLAG_SKIP_CAP
    if c["has_act"]:
        pl = c["planted_an"]
        assert pl.any() and (ref["actn"][pl] == 0.5).all() and not ref["flag"].transpose(0, 2, 1)[pl].any()
        assert cmp.transpose(0, 2, 1)[pl].all()                                             # exact: never left out
        hot = ref["score"].transpose(0, 2, 1)[pl].max(-1) > 1.5 * c["conf_thresh"]
        assert hot.any()                                                                    # flag 0 whatever the score
        if (~pl).any():                         # no other anchor within the actionness tolerance of 0.5
            assert ref["d_an"][~pl].min() > IC.ACTN_TOL[1] + IC.ACTN_TOL[0] * 0.5
    if N < 128:
        return
    assert 0.02 < ref["flag"].mean() < 0.98
    lo, hi, elo, ehi, rev = IC.clamp_counts(c)
    assert min(lo, hi, elo, ehi) >= IC.CLAMP_MIN and rev >= IC.CLAMP_MIN, (lo, hi, elo, ehi, rev)
    z = np.concatenate([c["inputs"]["conf"].reshape(-1), c["inputs"]["prop_conf"].reshape(-1)])
    up = lambda x, to: np.nextafter(np.float32(x), np.float32(to))
    for v in (10.0, up(10, 20), -10.0, up(-10, -20), 80.0, -80.0, 1e4, -1e4, 20.0, up(20, 30), up(20, 0)):
        assert (z == np.float32(v)).any(), v
    rows = c["inputs"]["conf"].reshape(N, K)
    assert ((rows < 0).all(1)).sum() >= 8 and ((rows == rows[:, :1]).all(1)).sum() >= 4     # all-negative, all-equal rows
    near = c["near"]
    assert len(near) >= 8
    s = ref["score"].transpose(0, 2, 1).reshape(N, -1)[near, c["near_class"]]
    rel = s / np.float32(c["conf_thresh"]) - 1.0
    assert (np.abs(np.abs(rel) - IC.NEAR_THRESH) < 0.1 * IC.NEAR_THRESH).all() and (rel > 0).any() and (rel < 0).any()
    assert cmp.transpose(0, 2, 1).reshape(N, -1)[near, c["near_class"]].all()                             # compared, on both sides of the edge

"""References and deterministic cases of the inference post-processing kernels (csrc/infer.hip): the decode kernels
(otal_decode_clips, _ex, _ev) and the batched Soft-NMS (otal_softnms_classes, _ws).  numpy only, no GPU code here.

softnms_reference / decode_reference state the reference's rules (AFSD/common/segment_utils.py:128-162; AFSD/thumos14/test.py:79-162
with BDNet.py:538-561) in float64 on the float32 inputs.  tests/test_infer_cases_cpu.py proves them against the reference-generated
fixtures and asserts that every case has the structure it claims; tests/test_infer_edges_gpu.py runs the cases through the kernels.

Soft-NMS cases come in two kinds.  In the exact ones every decision of the kernel has exact operands: the segments that meet
have iou exactly 0 (the decay factor is exp(-0) = 1, scores never change) or exactly 1, so kept sets, counts and indices must equal
the reference with nothing excluded, ties included.  In the random ones (overlapping segments, scores through expf) the kernel may
deviate from float64 by NMS_UNITS * rounds * 2^-24 relative -- per round a few fp32 operations on iou, whose error the exponent
x = -iou^2 / sigma amplifies by |x| <= 1 / sigma <= 2, one expf and one multiply -- and a seed is admitted only when
the reference's decision margin (the smallest relative gap between the best and the second-best undone score of a round, and of any
initial or decayed score to the threshold) is at least NMS_SAFETY times that bound: the seeds below were picked on the CPU until
that held, so no case is left out on the GPU.

Decode cases: flags are decisions on fp32 scores, so an element is compared only where the float64 score is farther from conf_thresh
(and the actionness from 0.5) than the score tolerance; the CPU test caps the share left out at FLAG_SKIP_CAP per case.  Anchors
planted with act = prop_act = 0 have actionness exactly 0.5 in fp32 (1 / (1 + exp(-0)) = 0.5), `an > 0.5` is false there whatever
the score, and they are never left out."""
import functools

import numpy as np

U = 2.0 ** -24
F32 = np.float32

# ------------------------------------------------------------------------------------------------ Soft-NMS: the reference
NMS_UNITS = 16              # kernel's relative deviation from float64 after r rounds <= NMS_UNITS * r * 2^-24
NMS_SAFETY = 4              # margin / bound a random case needs, and rtol / bound of the decayed scores
LDS_ROWS = 7680             # NMS_LDS_LIMIT / 20 of csrc/infer.hip: the largest working set that runs from LDS


def nms_bound(rounds):
    return NMS_UNITS * max(int(rounds), 1) * U


def softnms_reference(rows, sigma, top_k, thr):
    """softnms_v2 (segment_utils.py:128-162) in float64 on fp32 rows [start, end, score, ...], thr and sigma rounded to fp32.
    -> dict(kept (n) bool, score (n) float64 decayed scores, rounds, margin)."""
    rows = np.asarray(rows, F32)
    sigma, thr, min_width = float(F32(sigma)), float(F32(thr)), float(F32(1e-5))
    ts, te, sc = (rows[:, i].astype(np.float64) for i in range(3))
    n = rows.shape[0]
    undone = sc >= thr                                  # candidates: score >= thr
    done = np.zeros(n, bool)
    margin = float(np.min(np.abs(sc - thr) / thr)) if n else np.inf
    rounds = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        while undone.sum() > 1 and done.sum() < top_k:
            idx = np.nonzero(undone)[0]
            s = sc[idx]
            o = int(np.argmax(s))                       # the first maximum wins
            j = idx[o]
            margin = min(margin, float((s[o] - np.max(np.delete(s, o))) / s[o]))
            undone[j], done[j] = False, True
            rounds += 1
            u = np.nonzero(undone)[0]
            a, b = ts[u], te[u]
            inter = np.maximum(np.minimum(b, te[j]) - np.maximum(a, ts[j]), 0.0)
            width = max(te[j] - ts[j], min_width)
            iou = inter / (width + (b - a) - inter)
            sc[u] = sc[u] * np.exp(-iou ** 2 / sigma)
            margin = min(margin, float(np.min(np.abs(sc[u] - thr) / thr)))
            undone[u[sc[u] < thr]] = False
    return dict(kept=done, score=sc, rounds=rounds, margin=margin)


# ------------------------------------------------------------------------------------------------ Soft-NMS: batches and problems
def one_problem(rows):
    """(n, 5) rows [start, end, score, unct, actn] as a batch of one video with one clip of n anchors and one class, all flagged."""
    rows = np.ascontiguousarray(rows, F32)
    n = rows.shape[0]
    return dict(seg=rows[None, :, :2].copy(), score=rows[None, None, :, 2].copy(), unct=rows[None, :, 3].copy(),
                actn=rows[None, :, 4].copy(), flag=np.ones((1, 1, n), np.uint8), clip_start=[0, 1], A=n, K=1)


def problem(batch, v, k):
    """The candidates of (video v, class k) in the kernel's order (clip-major, anchor-minor): rows (m, 5) and their source index
    clip * A + anchor relative to the video's first clip."""
    c0, c1 = batch["clip_start"][v], batch["clip_start"][v + 1]
    src = np.nonzero(batch["flag"][c0:c1, k].reshape(-1))[0]
    col = lambda a: a[c0:c1].reshape(-1)[src][:, None]
    rows = np.concatenate([batch["seg"][c0:c1].reshape(-1, 2)[src], col(batch["score"][:, k]), col(batch["unct"]),
                           col(batch["actn"])], 1).astype(F32)
    return rows, src.astype(np.int32)


def problems(batch):
    V, K = len(batch["clip_start"]) - 1, batch["K"]
    return [(v, k) for v in range(V) for k in range(K)]


def _rest(rs, n):
    return rs.uniform(0, 1, n).astype(F32), rs.uniform(0.3, 1, n).astype(F32)


def _disjoint_rows(rs, scores):
    """Segment i = [3 i, 3 i + 1 + u_i], u in [0, 1): pairwise disjoint, iou exactly 0."""
    n = len(scores)
    start = 3.0 * np.arange(n)
    unct, actn = _rest(rs, n)
    return np.stack([start, start + 1.0 + rs.uniform(0, 1, n), scores, unct, actn], 1).astype(F32)


def is_disjoint(rows):
    o = np.argsort(rows[:, 0], kind="stable")
    return bool((rows[:, 1] > rows[:, 0]).all() and (rows[o[1:], 0] > rows[o[:-1], 1]).all())


TIE_VALUES = (0.75, 0.5, 0.3125, 0.125)
TIE_TOP_K = (1, 7, 255, 256, 257, 999, 1000, 5000)
TIE_FIRST = 69          # the first maximum: thread 69 of wave 1; equal scores planted in its stride, its wave and the other waves


def _ties():
    rs = np.random.RandomState(7)
    sc = np.asarray(TIE_VALUES, F32)[rs.randint(0, 4, 1000)]
    sc[:TIE_FIRST][sc[:TIE_FIRST] == TIE_VALUES[0]] = TIE_VALUES[1]
    # same thread (i + 256, i + 512), same wave other lanes, waves 0 / 2 / 3 of the same sweep, and a later sweep
    sc[[TIE_FIRST, TIE_FIRST + 256, TIE_FIRST + 512, 70, 127, 128, 200, 255, 256 + 3, 512 + 64]] = TIE_VALUES[0]
    return _disjoint_rows(rs, sc)


def _all_equal():
    return _disjoint_rows(np.random.RandomState(8), np.full(513, 0.4375, F32))


THR = F32(0.001)


def _thr_equality():
    """12 distinct scores above thr, 15 exactly thr (candidates, and `s < thr` is false for them in every round), 15 one ulp below
    (never candidates), interleaved."""
    rs = np.random.RandomState(9)
    sc = np.concatenate([np.linspace(0.2, 0.9, 12).astype(F32), np.full(15, THR, F32),
                         np.full(15, np.nextafter(THR, F32(0)), F32)])
    return _disjoint_rows(rs, sc[rs.permutation(len(sc))])


DUP_THR = F32(0.1)
DUP_SEEDS = {0.5: 255, 0.85: 71}


def _duplicates(sigma):
    """14 groups of 3 identical segments (iou exactly 1 inside a group, 0 across): a member decays by exp(-1 / sigma) once or twice."""
    rs = np.random.RandomState(100 + DUP_SEEDS[sigma])
    g = np.repeat(np.arange(14), 3)
    start = 10.0 * g
    sc = rs.uniform(0.1, 0.95, len(g)).astype(F32)
    unct, actn = _rest(rs, len(g))
    rows = np.stack([start, start + 4.0, sc, unct, actn], 1).astype(F32)
    return rows[rs.permutation(len(g))]


def random_rows(rs, n):
    """The overlapping candidates of the random cases: uniform centres in [5, 90], widths |N(6, 3)| + 0.5, scores
    0.05 + 0.9 Beta(0.5, 2)."""
    c = rs.uniform(5, 90, n)
    w = np.abs(rs.normal(6, 3, n)) + 0.5
    sc = 0.05 + 0.9 * rs.beta(0.5, 2.0, n)
    unct, actn = _rest(rs, n)
    return np.stack([c - w / 2, c + w / 2, sc, unct, actn], 1).astype(F32)


DEGENERATE_SEED = 3


def _degenerate():
    """64 random overlapping candidates of which 8 have zero width and 8 have end < start (decode clamps the two ends
    independently).  A reversed candidate never intersects anything and a zero-width one has inter = 0: their iou is +-0 as long
    as width + (end - start) != 0, which holds here (|end - start| >= 0.25, zero-width tops get width 1e-5)."""
    rs = np.random.RandomState(200 + DEGENERATE_SEED)
    rows = random_rows(rs, 64)
    pick = rs.permutation(64)[:16]
    rows[pick[:8], 1] = rows[pick[:8], 0]                                   # zero width
    rows[pick[8:], 1] = rows[pick[8:], 0] - rs.uniform(0.25, 6, 8).astype(F32)     # end < start
    return rows


def _boundary_rows(n):
    """n disjoint candidates with distinct scores, the two highest in the last two rows and the third in row 0."""
    rs = np.random.RandomState(n)
    sc = (0.1 + 0.7 * rs.permutation(n) / n).astype(F32)
    sc[0], sc[-2], sc[-1] = 0.85, 0.9, 0.95
    return _disjoint_rows(rs, sc)


def _batch(seed, A, K, clips, density, empty_clips=(), empty_classes=(), low=0.0005):
    """Disjoint segments inside a video (row r of the video: [3 r, 3 r + 1 + u]), distinct scores per (clip, class, anchor) in
    [low, 1), flags drawn with `density` independently of the scores."""
    rs = np.random.RandomState(seed)
    cs = np.concatenate([[0], np.cumsum(clips)]).astype(int).tolist()
    n = cs[-1]
    seg = np.zeros((n, A, 2), F32)
    for v in range(len(clips)):
        m = clips[v] * A
        start = 3.0 * np.arange(m)
        seg[cs[v]:cs[v + 1]] = np.stack([start, start + 1.0 + rs.uniform(0, 1, m)], 1).reshape(clips[v], A, 2)
    score = (low + (1 - low) * (rs.permutation(n * K * A) + 0.5) / (n * K * A)).astype(F32).reshape(n, K, A)
    flag = (rs.uniform(0, 1, (n, K, A)) < density).astype(np.uint8)
    for c in empty_clips:
        flag[c] = 0
    for k in empty_classes:
        flag[:, k] = 0
    return dict(seg=seg, score=score, unct=rs.uniform(0, 1, (n, A)).astype(F32), actn=rs.uniform(0.3, 1, (n, A)).astype(F32),
                flag=flag, clip_start=cs, A=A, K=K)


# A -> clips per video: a 256-row chunk of the gather covers 256 clips (A = 1), 51.2 clips (5), two whole clips and a part of
# a third (126), or lies inside one clip / straddles two (300)
LAYOUT = {1: [300, 0, 7], 5: [120, 3, 0, 60], 126: [5, 1, 3], 300: [3, 2]}
LAYOUT_EMPTY_CLIPS = {1: (5, 6, 301), 5: (0, 51, 52, 121), 126: (1, 5), 300: (3,)}
BOUNDARY_CLIPS = [60, 61, 0, 1]          # A = 128: 7680 rows (exactly the LDS working set), 7808 (scratch), none, 128
RANDOM_SEEDS = {(64, 0.5): 0, (64, 0.85): 1, (150, 0.5): 2, (150, 0.85): 2, (300, 0.5): 14, (300, 0.85): 22}
RANDOM_TOP_K = (20, 5000)

# name -> dict(batch, sigma, top_k, thr, exact): `exact` = scores never change (bit-for-bit rows); else rtol from the rounds
NMS_CASES = {}
for _t in TIE_TOP_K:
    NMS_CASES[f"ties-top{_t}"] = dict(make=lambda: one_problem(_ties()), sigma=0.5, top_k=_t, thr=THR, exact=True)
NMS_CASES["all_equal"] = dict(make=lambda: one_problem(_all_equal()), sigma=0.5, top_k=100, thr=THR, exact=True)
NMS_CASES["thr_equality"] = dict(make=lambda: one_problem(_thr_equality()), sigma=0.5, top_k=5000, thr=THR, exact=True)
for _s in (0.5, 0.85):
    NMS_CASES[f"duplicates-s{_s}"] = dict(make=functools.partial(lambda s: one_problem(_duplicates(s)), _s), sigma=_s, top_k=5000,
                                          thr=DUP_THR, exact=False)
NMS_CASES["degenerate"] = dict(make=lambda: one_problem(_degenerate()), sigma=0.5, top_k=5000, thr=THR, exact=False)
for _a in LAYOUT:
    NMS_CASES[f"layout-A{_a}"] = dict(make=functools.partial(lambda a: _batch(300 + a, a, 3, LAYOUT[a], 0.3, LAYOUT_EMPTY_CLIPS[a],
                                                                              (1,)), _a),
                                      sigma=0.5, top_k=5000, thr=THR, exact=True)
    NMS_CASES[f"isolation-A{_a}"] = dict(NMS_CASES[f"layout-A{_a}"], top_k=5)
NMS_CASES["boundary_batch"] = dict(make=lambda: _batch(400, 128, 2, BOUNDARY_CLIPS, 1.0), sigma=0.5, top_k=64, thr=THR, exact=True)
for (_n, _s), _seed in RANDOM_SEEDS.items():
    for _t in RANDOM_TOP_K:
        NMS_CASES[f"random-n{_n}-s{_s}-top{_t}"] = dict(
            make=functools.partial(lambda n, seed: one_problem(random_rows(np.random.RandomState(seed), n)), _n, _seed),
            sigma=_s, top_k=_t, thr=THR, exact=False)
RANDOM_CASES = [k for k in NMS_CASES if k.startswith("random-")]
MARGIN_CASES = RANDOM_CASES + ["degenerate", "duplicates-s0.5", "duplicates-s0.85"]
BOUNDARY_ROWS = (LDS_ROWS, LDS_ROWS + 1)
BOUNDARY_TOP_K = 64


@functools.lru_cache(maxsize=None)
def nms_case(name):
    c = NMS_CASES[name]
    return dict(c, batch=c["make"](), name=name)


@functools.lru_cache(maxsize=None)
def nms_references(name):
    """{(v, k): (rows, src, softnms_reference(rows))} of a case."""
    c = nms_case(name)
    out = {}
    for v, k in problems(c["batch"]):
        rows, src = problem(c["batch"], v, k)
        out[(v, k)] = (rows, src, softnms_reference(rows, c["sigma"], c["top_k"], c["thr"]))
    return out


@functools.lru_cache(maxsize=None)
def boundary_rows(n):
    rows = _boundary_rows(n)
    return rows, softnms_reference(rows, 0.5, BOUNDARY_TOP_K, THR)


# ------------------------------------------------------------------------------------------------ decode: the reference
SEG_TOL = (1e-6, 1e-5)          # rtol, atol of tests/test_infer_gpu.py
ACTN_TOL = (1e-5, 1e-7)
SCORE_ATOL = 1e-7
FLAG_SKIP_CAP = 0.005
EXP, RELU, SOFTPLUS = 0, 1, 2


def score_rtol(K):
    """score and unct: the sequential fp32 sum over K terms."""
    return max(1e-5, 2 * K * U)


def _evidence(z, kind):
    if kind == RELU:
        return np.maximum(z, 0.0)
    if kind == SOFTPLUS:                                    # F.softplus: beta 1, threshold 20
        return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))
    return np.exp(np.clip(z, -10.0, 10.0))


def decode_reference(inputs, clip_length, conf_thresh, score_fn, first_class, evidence, has_act):
    """parse_output + decode_predictions + the threshold test of filtering (test.py:79-162) in float64 on the fp32 inputs.
    inputs: loc, prop_loc (n, A, 2); priors (A[, 1]); conf, prop_conf (n, A, K); center (n, A[, 1]); act, prop_act (n, A[, 1]) with
    has_act; offsets, fps (n).  score_fn 0: Dirichlet mean of alpha = evidence + 1 (BDNet.py:538-561), uncertainty K / S averaged
    over the two stages; 1: softmax, uncertainty 0.  -> dict(seg (n, A, 2), score (n, K - first_class, A), unct, actn (n, A),
    flag, d_score = |score - conf_thresh|, d_an = |actionness - 0.5| (inf without the actionness heads))."""
    f = lambda k: np.asarray(inputs[k], F32).astype(np.float64)
    loc, ploc, conf, pconf = f("loc"), f("prop_loc"), f("conf"), f("prop_conf")
    n, A, K = conf.shape
    clip, thr = float(F32(clip_length)), float(F32(conf_thresh))
    w = loc[..., 0] + loc[..., 1]
    r0, r1 = 0.5 * w * ploc[..., 0] + loc[..., 0], 0.5 * w * ploc[..., 1] + loc[..., 1]
    pc = f("priors").reshape(1, A) * clip
    off, fps = f("offsets").reshape(n, 1), f("fps").reshape(n, 1)
    seg = np.stack([(np.clip(pc - r0, 0.0, clip) + off) / fps, (np.clip(pc + r1, 0.0, clip) + off) / fps], -1)

    def probs(z):
        if score_fn == 1:
            e = np.exp(z - z.max(-1, keepdims=True))
            return e / e.sum(-1, keepdims=True), np.zeros(z.shape[:-1])
        alpha = _evidence(z, evidence) + 1.0
        S = alpha.sum(-1, keepdims=True)
        return alpha / S, K / S[..., 0]

    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    (p, u), (pp, pu) = probs(conf), probs(pconf)
    an = (sig(f("act").reshape(n, A)) + sig(f("prop_act").reshape(n, A))) / 2.0 if has_act else np.zeros((n, A))
    score = (p + pp) / 2.0 * sig(f("center").reshape(n, A))[..., None]
    if has_act:
        score = score * an[..., None]
    score = np.ascontiguousarray(score[..., first_class:].transpose(0, 2, 1))
    flag = score > thr
    if has_act:
        flag &= (an > 0.5)[:, None, :]
    return dict(seg=seg, score=score, unct=(u + pu) / 2.0, actn=an, flag=flag, d_score=np.abs(score - thr),
                d_an=np.abs(an - 0.5) if has_act else np.full((n, A), np.inf))


def flags_compared(ref, K, planted_an=None):
    """bool (n, KO, A): the flags a float32 decode must reproduce -- both decisions farther from their edge than the score
    tolerance at that element, plus every anchor planted with actionness exactly 0.5."""
    tol = SCORE_ATOL + score_rtol(K) * np.abs(ref["score"])
    ok = (ref["d_score"] > tol) & (ref["d_an"][:, None, :] > tol)
    if planted_an is not None:
        ok |= planted_an[:, None, :]
    return ok


# ------------------------------------------------------------------------------------------------ decode: the cases
# name -> (score_fn, first_class, evidence, has_act)
CONFIGS = {"opental_exp": (0, 0, EXP, True), "opental_relu": (0, 0, RELU, True), "opental_softplus": (0, 0, SOFTPLUS, True),
           "closed_exp": (0, 1, EXP, False), "closed_relu": (0, 1, RELU, False), "closed_softplus": (0, 1, SOFTPLUS, False),
           "closed_softmax": (1, 1, EXP, False)}
SHAPES = {0: [(1, 1, 1), (3, 128, 15), (2, 129, 16), (2, 300, 151), (1, 189, 201)],
          1: [(2, 1, 2), (3, 128, 15), (2, 129, 16), (2, 300, 151), (1, 189, 201)]}
CONF_THRESH = {1: 0.3, 2: 0.1, 15: 0.01, 16: 0.01, 151: 0.002, 201: 0.002}
CLIP_LENGTH = 256.0
OFFSETS, FPS = (0.0, 384.0, 12345.0), (10.0, 25.5, 29.97)
DECODE_CASES = [f"{cfg}-{n}x{A}x{K}" for cfg, c in CONFIGS.items() for n, A, K in SHAPES[c[1]]]
NEAR_THRESH = 3e-4          # planted scores sit at conf_thresh (1 +- NEAR_THRESH): >= 4 x the score tolerance away
CLAMP_MIN = 8               # anchors on each of the four clamps in every case with at least 128 anchors


def _planted_rows(K):
    up = lambda x, to: np.nextafter(F32(x), F32(to))
    one_hot = lambda hi, lo: np.concatenate([[hi], np.full(K - 1, lo)])
    t20 = np.array([20.0, up(20, 30), up(20, 0)], F32)
    t10 = np.array([10.0, up(10, 20), -10.0, up(-10, -20)], F32)
    return [np.full(K, 10.0), np.full(K, up(10, 20)), np.full(K, -10.0), np.full(K, up(-10, -20)), t10[np.arange(K) % 4],
            one_hot(80.0, -80.0), one_hot(-80.0, 80.0), one_hot(1e4, -1e4), one_hot(-1e4, 1e4), np.full(K, 1e4), np.full(K, -1e4),
            np.full(K, 3.25), t20[np.arange(K) % 3], np.full(K, up(20, 30)), np.full(K, up(20, 0))]


@functools.lru_cache(maxsize=None)
def decode_case(name):
    cfg, shape = name.split("-")
    score_fn, first_class, evidence, has_act = CONFIGS[cfg]
    n, A, K = (int(x) for x in shape.split("x"))
    rs = np.random.RandomState(1000 + 7 * n + 11 * A + 13 * K + 17 * list(CONFIGS).index(cfg))
    t = lambda *s, scale=1.0: (rs.randn(*s) * scale).astype(F32)
    ins = dict(loc=(20.0 + 150.0 * rs.randn(n, A, 2)).astype(F32), prop_loc=t(n, A, 2, scale=0.3), conf=t(n, A, K, scale=6.0),
               prop_conf=t(n, A, K, scale=6.0), center=t(n, A), priors=((np.arange(A) + 0.5) / A).astype(F32),
               offsets=np.array([OFFSETS[(c + A) % 3] for c in range(n)], F32),
               fps=np.array([FPS[(c + K) % 3] for c in range(n)], F32))
    if has_act:
        ins["act"], ins["prop_act"] = t(n, A), t(n, A)
    N = n * A
    conf, pconf, center = ins["conf"].reshape(N, K), ins["prop_conf"].reshape(N, K), ins["center"].reshape(N)
    rows = _planted_rows(K)
    for j in range(min(N, 2 * len(rows))):              # planted logit rows: both stages, then the refined stage alone
        pconf[j] = rows[j % len(rows)]
        if j < len(rows):
            conf[j] = rows[(j + (j % 2)) % len(rows)]
    free = np.arange(2 * len(rows), N)
    neg = free[:16]                                     # all-negative rows: relu gives alpha = 1 everywhere
    conf[neg], pconf[neg] = -np.abs(conf[neg]) - F32(0.5), -np.abs(pconf[neg]) - F32(0.5)
    planted_an = np.zeros(N, bool)
    if has_act:
        planted_an[np.arange(0, N, 7)] = True           # act = prop_act = 0: actionness exactly 0.5
        if N > 16:
            planted_an[:3] = False
        act, pact = ins["act"].reshape(N), ins["prop_act"].reshape(N)
        act[planted_an], pact[planted_an] = 0.0, 0.0
        hot = np.nonzero(planted_an)[0][::2]            # half of them with a score well above the threshold
        hot = hot[hot >= 2 * len(rows)] if N > 2 * len(rows) else hot
        conf[hot], pconf[hot], center[hot] = 0.0, 0.0, 6.0
        conf[hot, first_class], pconf[hot, first_class] = 9.0, 9.0
    case = dict(name=name, inputs=ins, clip_length=CLIP_LENGTH, conf_thresh=CONF_THRESH[K], score_fn=score_fn,
                first_class=first_class, evidence=evidence, has_act=has_act, planted_an=planted_an.reshape(n, A), shape=(n, A, K))
    # scores planted next to conf_thresh: the centre logit that puts the anchor's best class at conf_thresh (1 +- NEAR_THRESH)
    near = free[16:32][~planted_an[free[16:32]]]
    case["near"], case["near_class"] = near, np.zeros(len(near), int)
    if len(near):
        sc = reference_of(case)["score"].transpose(0, 2, 1).reshape(N, -1)[near]
        cls = sc.argmax(1)
        base = sc[np.arange(len(near)), cls] * (1.0 + np.exp(-center[near].astype(np.float64)))       # the score at sigmoid(center) = 1
        want = case["conf_thresh"] * (1.0 + NEAR_THRESH * np.where(np.arange(len(near)) % 2, 1.0, -1.0)) / np.maximum(base, 1e-300)
        ok = (want > 1e-4) & (want < 1 - 1e-4)
        center[near[ok]] = np.log(want[ok] / (1.0 - want[ok])).astype(F32)
        case["near"], case["near_class"] = near[ok], cls[ok]
    return case


def reference_of(case):
    return decode_reference(case["inputs"], case["clip_length"], case["conf_thresh"], case["score_fn"], case["first_class"],
                            case["evidence"], case["has_act"])


@functools.lru_cache(maxsize=None)
def decode_ref(name):
    return reference_of(decode_case(name))


def clamp_counts(case):
    """Anchors on each of the four segment clamps (start at 0, start at clip_length, end at 0, end at clip_length) and anchors
    with end < start, in float64."""
    i = {k: np.asarray(v, np.float64) for k, v in case["inputs"].items()}
    clip = case["clip_length"]
    w = i["loc"][..., 0] + i["loc"][..., 1]
    s0 = i["priors"].reshape(1, -1) * clip - (0.5 * w * i["prop_loc"][..., 0] + i["loc"][..., 0])
    s1 = i["priors"].reshape(1, -1) * clip + (0.5 * w * i["prop_loc"][..., 1] + i["loc"][..., 1])
    rev = np.clip(s1, 0, clip) < np.clip(s0, 0, clip)
    return int((s0 < 0).sum()), int((s0 > clip).sum()), int((s1 < 0).sum()), int((s1 > clip).sum()), int(rev.sum())

"""The dataset-independent half of the inference path on MI355X, with the reference's function names
(AFSD/thumos14/test.py): get_offsets (:48-56), parse_output (:79-109), decode_predictions (:112-140), filtering (:143-162),
get_video_detections (:165-200).

`detect` is the MI355X-first pipeline every driver runs: all sliding windows of a batch of videos go through the network in
large batches (the reference runs b=1, test.py:227-235), then TWO launches do the rest -- a decode launch (decode + per-class
threshold for every clip; the caller says which) and otal_softnms_classes (gather + Soft-NMS for every (video, class)) --
with no host synchronisation until the final copy.  thumos14/test.py, thumos14/test_openmax.py and anet/test.py each call it
with their own decode; the proposal dicts, the result-file layout and the known/unknown threshold of the drivers live here
too.  Multi-GPU: shard the video list across ranks (as the reference's unused AFSD/anet/test.py:248-273 sketches); there is
no collective on this path, `gather_results` collects the dicts afterwards.
"""

import torch

from .. import _lib as L
from .ops import EVIDENCE


def get_offsets(sample_count, clip_length, stride):
    """test.py:48-56 with the video's sample count passed in."""
    if sample_count < clip_length:
        return [0]
    out = list(range(0, sample_count - clip_length + 1, stride))
    if (sample_count - clip_length) % stride:
        out += [sample_count - clip_length]
    return out


_WINDOW_DTYPE = None


def prepare_windows(videos, windows, clip_length):
    """All windows of one forward pass in ONE launch (otal_prepare_windows): videos = uint8 (C,Tv,H,W) device tensors,
    windows = [(video index, offset)].  Bit-identical to torch.cat([prepare_clip(videos[v], o, clip_length) ...])."""
    import numpy as np
    global _WINDOW_DTYPE
    if _WINDOW_DTYPE is None:
        _WINDOW_DTYPE = np.dtype([("src", "<u8"), ("chan_stride4", "<i4"), ("valid_t", "<i4")])
    C, _, H, W = videos[windows[0][0]].shape
    recs = np.zeros(len(windows), _WINDOW_DTYPE)
    for i, (v, o) in enumerate(windows):
        d = videos[v]
        if d.dtype != torch.uint8 or not d.is_cuda or not d.is_contiguous() or tuple(d.shape[2:]) != (H, W) or d.shape[0] != C:
            raise RuntimeError("videos must be contiguous uint8 (C,T,H,W) device tensors of one frame size")
        if (H * W) % 4 or d.data_ptr() % 4 or not 0 <= o < d.shape[1]:
            raise RuntimeError("otal_prepare_windows needs H*W % 4 == 0, 4-byte aligned videos and offsets inside the video")
        recs[i] = (d.data_ptr() + o * H * W, d.shape[1] * H * W // 4, min(clip_length, d.shape[1] - o))
    dev = videos[windows[0][0]].device
    params = torch.from_numpy(recs.view(np.uint8).copy()).to(dev, non_blocking=True)
    out = torch.empty((len(windows), C, clip_length, H, W), dtype=torch.float32, device=dev)
    L.check(L.lib().otal_prepare_windows(L.ptr(params), L.ptr(out), len(windows), C, clip_length, H, W, L.stream()),
            "otal_prepare_windows")
    return out


def head_mode(net):
    """(os_head, use_edl, evidence) of a BDNet: which decode its outputs need.  A network that does not say is
    taken for the OpenTAL head (os_head, use_edl, exp evidence)."""
    return bool(getattr(net, 'os_head', True)), bool(getattr(net, 'use_edl', True)), getattr(net, 'evidence', 'exp')


def rpl_logits(output_dict, use_gcpl=False):
    """The classification maps the closed-set softmax decode reads for the distance head (parse_output, test.py:85-87): the
    distances themselves for RPL, their negation for GCPL.  Host or device tensors.
    Applied to the (fused) maps: both streams' maps are distances, so a two-stream GCPL run scores softmax(-(rgb + flow) / 2).
    Reference hazard: its parse_output negates the rgb stream BEFORE the average and leaves the flow stream as it is
    (test.py:85-87 then :96-99), i.e. softmax((flow - rgb) / 2) -- pinned in tests/golden/rpl.npz (dec_gcpl_fus1_*) and
    reproduced in tests/test_rpl_gpu.py, not adopted.  Single-stream runs are unaffected."""
    if not use_gcpl:
        return output_dict
    return dict(output_dict, conf=-output_dict['conf'], prop_conf=-output_dict['prop_conf'])


def clip_scalars(offsets, fps, n, dev):
    """The per-clip scalars of the decode kernels as fp32 device tensors of n entries: offsets (n), and fps, which may be
    one value for all clips."""
    offs = torch.as_tensor(offsets, dtype=torch.float32, device=dev).contiguous()
    fpst = torch.as_tensor(fps, dtype=torch.float32, device=dev).contiguous()
    if fpst.numel() == 1:
        fpst = fpst.expand(n).contiguous()
    return offs, fpst


def decode_clips(output_dict, offsets, fps, clip_length=256, conf_thresh=0.01, os_head=True, use_edl=True, evidence='exp',
                 use_gcpl=False):
    """Batched parse_output + decode_predictions + threshold masks.  output_dict: model outputs for
    `n` clips; offsets/fps: per-clip tensors or lists.  Returns dict(seg, score, unct, actn, flag).
    os_head / use_edl / evidence: the network's head (head_mode).  The closed-set head (os_head False) has a background
    logit, which score / flag leave out (K - 1 classes); unct is None without use_edl, actn None without os_head.
    Evidence other than 'exp' goes through otal_decode_clips_ev."""
    if use_edl and evidence not in EVIDENCE:
        raise NotImplementedError(f"evidence {evidence!r}: the decode kernel computes {', '.join(EVIDENCE)} evidence")
    if use_edl and evidence != 'exp' and not output_dict['loc'].is_cuda:
        # otal_decode_clips_ev reads device memory: a host pointer must not reach it, and there is no host form of this decode
        raise NotImplementedError(f"evidence {evidence!r} on host tensors: otal_decode_clips_ev decodes device tensors only")
    if os_head and not use_edl:
        raise NotImplementedError("an actionness head with softmax scores is not a THUMOS14 configuration")
    if use_gcpl and (os_head or use_edl):
        raise NotImplementedError("use_gcpl belongs to the closed-set softmax decode of the distance head")
    output_dict = rpl_logits(output_dict, use_gcpl)
    loc = output_dict['loc'].contiguous()
    n, A, _ = loc.shape
    K = output_dict['conf'].shape[-1]
    if not os_head:
        return _decode_clips_ex(output_dict, loc, offsets, fps, clip_length, conf_thresh, use_edl, evidence)
    dev = loc.device
    offs, fpst = clip_scalars(offsets, fps, n, dev)
    seg = torch.empty((n, A, 2), device=dev)
    score = torch.empty((n, K, A), device=dev)
    unct = torch.empty((n, A), device=dev)
    actn = torch.empty((n, A), device=dev)
    flag = torch.empty((n, K, A), dtype=torch.uint8, device=dev)
    t = lambda k: output_dict[k].contiguous()
    head = (L.ptr(loc), L.ptr(t('prop_loc')), L.ptr(output_dict['priors'].contiguous()), L.ptr(t('conf')), L.ptr(t('prop_conf')),
            L.ptr(t('center')), L.ptr(t('act')), L.ptr(t('prop_act')), L.ptr(offs), L.ptr(fpst), L.ptr(seg), L.ptr(score),
            L.ptr(unct), L.ptr(actn), L.ptr(flag), n, A, K, clip_length, conf_thresh)
    if evidence == 'exp':
        L.check(L.lib().otal_decode_clips(*head, L.stream()), "otal_decode_clips")
    else:
        L.check(L.lib().otal_decode_clips_ev(*head, 0, 0, EVIDENCE[evidence], L.stream()), "otal_decode_clips_ev")
    return dict(seg=seg, score=score, unct=unct, actn=actn, flag=flag)


def _decode_clips_ex(output_dict, loc, offsets, fps, clip_length, conf_thresh, use_edl, evidence='exp'):
    """The closed-set head: otal_decode_clips_ex with softmax (score_fn 1) or Dirichlet (0) scores, class 0 dropped and
    no actionness (test.py:112-162 with os_head False); Dirichlet scores of relu / softplus evidence: otal_decode_clips_ev."""
    n, A, _ = loc.shape
    K = output_dict['conf'].shape[-1]
    dev = loc.device
    offs, fpst = clip_scalars(offsets, fps, n, dev)
    seg = torch.empty((n, A, 2), device=dev)
    score = torch.empty((n, K - 1, A), device=dev)
    unct = torch.empty((n, A), device=dev) if use_edl else None
    flag = torch.empty((n, K - 1, A), dtype=torch.uint8, device=dev)
    t = lambda k: output_dict[k].contiguous()
    head = (L.ptr(loc), L.ptr(t('prop_loc')), L.ptr(output_dict['priors'].contiguous()), L.ptr(t('conf')), L.ptr(t('prop_conf')),
            L.ptr(t('center')), None, None, L.ptr(offs), L.ptr(fpst), L.ptr(seg), L.ptr(score),
            None if unct is None else L.ptr(unct), None, L.ptr(flag), n, A, K, clip_length, conf_thresh,
            0 if use_edl else 1, 1)
    if use_edl and evidence != 'exp':
        L.check(L.lib().otal_decode_clips_ev(*head, EVIDENCE[evidence], L.stream()), "otal_decode_clips_ev")
    else:
        L.check(L.lib().otal_decode_clips_ex(*head, L.stream()), "otal_decode_clips_ex")
    return dict(seg=seg, score=score, unct=unct, actn=None, flag=flag)


_MAPS = ('loc', 'prop_loc', 'conf', 'prop_conf', 'center')
_ACT_MAPS = ('act', 'prop_act')
_UNCT_MAPS = ('unct', 'prop_unct')
_PRIORS_FOUND_EQUAL = []    # (a, b, a._version, b._version) of priors tensors compared once; a network hands out ONE priors tensor


def _same_priors(a, b):
    """Whether two networks' priors hold the same values.  Comparing reads the device once (torch.equal), so a pair found equal
    is remembered by identity and version: the batches of a run after the first do not synchronise with the host."""
    if a is b:
        return True
    for x, y, vx, vy in _PRIORS_FOUND_EQUAL:
        if x is a and y is b and (vx, vy) == (a._version, b._version):
            return True
    if a.shape != b.shape or not torch.equal(a, b):
        return False
    del _PRIORS_FOUND_EQUAL[:-7]        # a handful of network pairs at the most
    _PRIORS_FOUND_EQUAL.append((a, b, a._version, b._version))
    return True


def decode_clips_two_stream(rgb_out, flow_out, offsets, fps, clip_length=256, conf_thresh=0.01, os_head=True, use_edl=True,
                            evidence='exp', use_gcpl=False):
    """decode_clips for a two-stream run, from the two networks' RAW outputs in one launch (otal_decode_clips_2s): the kernel
    reads (rgb + flow) / 2 of every map in registers, so no averaged map is ever written.  Returns the dict of decode_clips:
    seg, score, actn and flag are bit for bit decode_clips(fuse_outputs(rgb_out, flow_out), ...)'s; unct, with use_edl, is the
    average of the networks' OWN uncertainty maps ((unct + prop_unct) / 2 of the fused outputs, parse_output test.py:105-108),
    shaped like them, which both outputs must then carry.  use_gcpl: the averaged distances are negated (rpl_logits on the fused
    maps).  Device tensors only; the head combinations decode_clips refuses are refused here, and so is a pair of outputs whose
    map shapes or priors differ."""
    if use_edl and evidence not in EVIDENCE:
        raise NotImplementedError(f"evidence {evidence!r}: the decode kernel computes {', '.join(EVIDENCE)} evidence")
    if os_head and not use_edl:
        raise NotImplementedError("an actionness head with softmax scores is not a THUMOS14 configuration")
    if use_gcpl and (os_head or use_edl):
        raise NotImplementedError("use_gcpl belongs to the closed-set softmax decode of the distance head")
    keys = _MAPS + (_ACT_MAPS if os_head else ()) + (_UNCT_MAPS if use_edl else ())
    for k in keys + ('priors',):
        a, b = rgb_out.get(k), flow_out.get(k)
        if a is None or b is None:
            raise RuntimeError(f"decode_clips_two_stream: both networks' outputs must carry '{k}'")
        if not (a.is_cuda and b.is_cuda) or a.dtype != torch.float32 or b.dtype != torch.float32:
            raise RuntimeError(f"decode_clips_two_stream decodes fp32 device tensors only ('{k}')")
        if a.shape != b.shape:
            raise RuntimeError(f"decode_clips_two_stream: '{k}' is {tuple(a.shape)} for rgb and {tuple(b.shape)} for flow")
    if not _same_priors(rgb_out['priors'], flow_out['priors']):
        raise RuntimeError("decode_clips_two_stream: the two networks have different priors")
    r = {k: rgb_out[k].contiguous() for k in keys}
    f = {k: flow_out[k].contiguous() for k in keys}
    n, A, _ = r['loc'].shape
    K = r['conf'].shape[-1]
    if r['prop_loc'].shape != (n, A, 2) or r['prop_conf'].shape != (n, A, K) or \
            any(r[k].numel() != n * A for k in keys if k not in ('loc', 'prop_loc', 'conf', 'prop_conf')):
        raise RuntimeError("decode_clips_two_stream: the maps are not those of %d clips x %d anchors x %d logits" % (n, A, K))
    if rgb_out['priors'].numel() != A:
        raise RuntimeError("decode_clips_two_stream: %d priors for %d anchors" % (rgb_out['priors'].numel(), A))
    dev = r['loc'].device
    offs, fpst = clip_scalars(offsets, fps, n, dev)
    if offs.numel() != n or fpst.numel() != n:
        raise RuntimeError("decode_clips_two_stream: offsets / fps are not one per clip")
    first = 0 if os_head else 1
    seg = torch.empty((n, A, 2), device=dev)
    score = torch.empty((n, K - first, A), device=dev)
    unct = torch.empty_like(r['unct']) if use_edl else None
    actn = torch.empty((n, A), device=dev) if os_head else None
    flag = torch.empty((n, K - first, A), dtype=torch.uint8, device=dev)
    opt = lambda d, k: L.ptr(d[k]) if k in d else None
    out = lambda v: None if v is None else L.ptr(v)
    L.check(L.lib().otal_decode_clips_2s(
        *[L.ptr(r[k]) for k in _MAPS], opt(r, 'act'), opt(r, 'prop_act'),
        *[L.ptr(f[k]) for k in _MAPS], opt(f, 'act'), opt(f, 'prop_act'),
        opt(r, 'unct'), opt(r, 'prop_unct'), opt(f, 'unct'), opt(f, 'prop_unct'),
        L.ptr(rgb_out['priors'].contiguous()), L.ptr(offs), L.ptr(fpst), L.ptr(seg), L.ptr(score), out(unct), out(actn),
        L.ptr(flag), n, A, K, clip_length, conf_thresh, 0 if use_edl else 1, first, EVIDENCE[evidence] if use_edl else 0,
        -1 if use_gcpl else 1, L.stream()), "otal_decode_clips_2s")
    return dict(seg=seg, score=score, unct=unct, actn=actn, flag=flag)


def decode_predictions(output_dict, idx, offset, sample_fps, clip_length=256, os_head=True, use_edl=True, evidence='exp',
                       use_gcpl=False):
    """Single-clip view with the reference's return values (test.py:112-140):
    decoded_segments (A,2), conf_scores (K,A), uncertainty (A,) or None, actionness (A,) or None.
    Closed-set heads: conf_scores holds the K - 1 non-background classes (row c = reference row c + 1)."""
    one = {k: (v[idx:idx + 1] if (v is not None and k != 'priors') else v) for k, v in output_dict.items()}
    d = decode_clips(one, [float(offset)], [float(sample_fps)], clip_length, os_head=os_head, use_edl=use_edl,
                     evidence=evidence, use_gcpl=use_gcpl)
    first = lambda v: None if v is None else v[0]
    return d['seg'][0], d['score'][0], first(d['unct']), first(d['actn'])


def filtering(decoded_segments, conf_score_cls, uncertainty, actionness, conf_thresh, use_edl=True, os_head=True):
    """test.py:143-162 for one class: (n, 3 + use_edl + os_head) rows [start,end,score(,unct)(,act)] or None."""
    m = conf_score_cls > conf_thresh
    if os_head:
        m = m & (actionness > 0.5)
    if int(m.sum()) == 0:
        return None
    cols = [decoded_segments[m], conf_score_cls[m, None]]
    if use_edl:
        cols.append(uncertainty[m, None])
    if os_head:
        cols.append(actionness[m, None])
    return torch.cat(cols, -1)


def softnms_classes(dec, clip_start, top_k=5000, sigma=0.5, score_threshold=0.001):
    """All (video, class) Soft-NMS problems in one launch.  clip_start: per-video clip ranges (V+1).
    Returns rows (V,K,top_k,cols), counts (V,K), index (V,K,top_k); cols = 3 + use_edl + os_head, i.e. 5 for the OpenTAL
    head ([start,end,score,unct,act]), 4 for the closed-set EDL and 3 for the Softmax baseline."""
    cols = 3 + (dec.get('unct') is not None) + (dec.get('actn') is not None)
    if dec.get('actn') is not None and dec.get('unct') is None:
        raise NotImplementedError("actionness rows without uncertainty")
    n, K, A = dec['score'].shape
    dev = dec['score'].device
    cs = torch.as_tensor(clip_start, dtype=torch.int32, device=dev).contiguous()
    V = cs.numel() - 1
    starts = [int(v) for v in clip_start]
    max_clips = max(b - a for a, b in zip(starts[:-1], starts[1:]))
    tk = min(int(top_k), max_clips * A)
    out = torch.zeros((V, K, tk, cols), device=dev)
    counts = torch.zeros((V, K), dtype=torch.int32, device=dev)
    index = torch.zeros((V, K, tk), dtype=torch.int32, device=dev)
    lib = L.lib()
    nbytes = lib.otal_softnms_scratch_bytes(n, max_clips, A, K)     # > 0: a video exceeds the LDS working set
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    opt = lambda v: None if v is None else L.ptr(v)
    L.check(lib.otal_softnms_classes_ws(L.ptr(dec['seg']), L.ptr(dec['score']), opt(dec.get('unct')),
                                        opt(dec.get('actn')), L.ptr(dec['flag']), L.ptr(cs), V, max_clips, A, K,
                                        sigma, tk, score_threshold, L.ptr(out), L.ptr(counts), L.ptr(index), cols,
                                        L.ptr(scratch), nbytes, n, L.stream()), "otal_softnms_classes_ws")
    return out, counts, index


def get_video_detections(rows, counts, idx_to_class=None, top_k=5000, duration=None, drop_empty=False):
    """test.py:165-200: per-video proposal list from the suppressed rows of one video (K,top_k,cols).  Rows of 3 or 4
    columns (closed-set heads) give 'uncertainty' / 'actionness' 0.0 where the column is absent (test.py:197-198).
    With `duration` (seconds) the cross-dataset and ActivityNet variant, test_cross_data.py:178-215 and
    anet/test.py:159-200: segments are clipped to [0, duration] and the ones left empty are dropped (`drop_empty` alone:
    the cross-dataset script's THUMOS14 leg, which passes no duration but still drops empty segments)."""
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    proposal_list = []
    for cl in range(rows.shape[0]):
        name = idx_to_class[cl + 1] if idx_to_class is not None else cl + 1
        for i in range(int(counts[cl])):
            r = rows[cl, i]
            if r[2] > 0:
                start, end = float(r[0]), float(r[1])
                if duration is not None or drop_empty:
                    start, end = max(0, start), (min(duration, end) if duration is not None else end)
                    if end <= start:
                        continue
                proposal_list.append({'label': name, 'score': float(r[2]), 'segment': [start, end],
                                      'uncertainty': float(r[3]) if len(r) > 3 else 0.0,
                                      'actionness': float(r[4]) if len(r) > 4 else 0.0})
    return proposal_list


# ----------------------------------------------------------------------------- the pipeline (test.py:203-252 without the JSON dump)
def enumerate_windows(videos, sample_fps, clip_length, stride):
    """The sliding windows of a batch of videos (uint8 (C,T,H,W) tensors): clips [(video index, offset)], and per clip its
    offset and fps as floats; clip_start (V+1) is each video's range of clips.  sample_fps: one value or one per video.
    stride None: one window at offset 0 per video (the ActivityNet recipe, where a video IS one clip)."""
    clips, offsets, fps, clip_start = [], [], [], [0]
    for v, data in enumerate(videos):
        offs = [0] if stride is None else get_offsets(data.shape[1], clip_length, stride)
        clips += [(v, o) for o in offs]
        offsets += [float(o) for o in offs]
        fps += [float(sample_fps[v] if hasattr(sample_fps, '__len__') else sample_fps)] * len(offs)
        clip_start.append(clip_start[-1] + len(offs))
    return clips, offsets, fps, clip_start


def fuse_outputs(rgb_out, flow_out):
    """Two-stream fusion by averaging the two networks' RAW outputs before decoding (parse_output, test.py:90-108): loc,
    conf, prop_loc, prop_conf, center, the actionness logits and -- with use_edl -- the two uncertainty maps.
    Reference hazard (H11): with os_head its parse_output squeezes the rgb actionness to (126,) but not the flow one
    ((126,1)), so `act + flow_act` broadcasts to (126,126) and decode_predictions fails on the OpenTAL configuration; the
    elementwise average it evidently means is what is computed here."""
    keys = ('loc', 'conf', 'prop_loc', 'prop_conf', 'center', 'act', 'prop_act', 'unct', 'prop_unct')
    fused = {k: (rgb_out[k] + flow_out[k]) / 2.0 for k in keys if rgb_out.get(k) is not None and flow_out.get(k) is not None}
    fused['priors'] = rgb_out['priors']
    return fused


def windows_per_pass(batch_clips):
    """The number of windows one forward pass takes when `batch_clips` are asked for."""
    # 32 windows per forward pass: past that the first feature maps leave the 32-bit buffer offsets of the vector-gather
    # kernels (64 windows: Conv3d_1a's output is 4.8 GB) and the generic kernels take over at half the speed
    return max(1, min(int(batch_clips), 32))


def forward_windows(net, videos, clips, clip_length, batch_clips, keys, flow_net=None, flow_videos=None, per_stream=False,
                    **net_kwargs):
    """The network over `clips` (enumerate_windows) in consecutive chunks of `batch_clips` windows -> its output maps named
    in `keys`, concatenated over the chunks ('priors' is the first pass's).  `flow_net` sees the same windows of
    `flow_videos`; the two networks' raw outputs are averaged per chunk (fuse_outputs), or with `per_stream` kept apart and
    returned as (rgb maps, flow maps) for a decode that reads both (decode_clips_two_stream).  net_kwargs go to the forward
    calls.  The chunking is part of the result: a forward pass of another batch size selects other conv kernels."""
    batch_clips = windows_per_pass(batch_clips)
    if per_stream and flow_net is None:
        raise RuntimeError("forward_windows: per_stream asks for a flow network")
    outs, flow_outs = [], []
    for i in range(0, len(clips), batch_clips):
        out = net(prepare_windows(videos, clips[i:i + batch_clips], clip_length), **net_kwargs)
        if flow_net is not None:
            flow_out = flow_net(prepare_windows(flow_videos, clips[i:i + batch_clips], clip_length), **net_kwargs)
            if per_stream:
                flow_outs.append(flow_out)
            else:
                out = fuse_outputs(out, flow_out)
        outs.append(out)
    merge = lambda parts: {k: (torch.cat([o[k] for o in parts], 0) if k != 'priors' else parts[0][k]) for k in keys}
    return (merge(outs), merge(flow_outs)) if per_stream else merge(outs)


@torch.no_grad()
def detect(net, videos, sample_fps, decode, keys, clip_length=256, stride=128, top_k=5000, nms_sigma=0.5, batch_clips=32,
           flow_net=None, flow_videos=None, decode_two_stream=None, two_stream_decode=True, **net_kwargs):
    """videos: list of uint8 (C,T,96,96) device tensors (already centre-cropped).  Every window through the network
    (enumerate_windows, forward_windows), then decode(merged outputs, offsets, fps) -> the dict of decode_clips, then the
    Soft-NMS launch.  Returns (rows, counts, index, dec); nothing synchronises with the host.
    With `flow_net` and a `decode_two_stream` callable the two networks' raw maps stay apart and
    decode_two_stream(rgb maps, flow maps, offsets, fps) decodes them (decode_clips_two_stream: one launch, no averaged
    copies); two_stream_decode=False, or no such callable, takes the earlier route: fuse_outputs per chunk, then `decode`."""
    clips, offsets, fps, clip_start = enumerate_windows(videos, sample_fps, clip_length, stride)
    if flow_net is not None and decode_two_stream is not None and two_stream_decode:
        rgb, flow = forward_windows(net, videos, clips, clip_length, batch_clips, keys, flow_net, flow_videos, True, **net_kwargs)
        dec = decode_two_stream(rgb, flow, offsets, fps)
    else:
        merged = forward_windows(net, videos, clips, clip_length, batch_clips, keys, flow_net, flow_videos, **net_kwargs)
        dec = decode(merged, offsets, fps)
    return softnms_classes(dec, clip_start, top_k, nms_sigma) + (dec,)


# ----------------------------------------------------------------------------- result files (test.py:246-252, threshold.py:128-150)
OOD_SCORES = {
    'uncertainty': lambda p: p['uncertainty'],
    'confidence': lambda p: 1 - p['score'],
    'uncertainty_actionness': lambda p: p['uncertainty'] * p['actionness'],
    'a_by_inv_u': lambda p: p['actionness'] / (1 - p['uncertainty'] + 1e-6),
    'u_by_inv_a': lambda p: p['uncertainty'] / (1 - p['actionness'] + 1e-6),
    'half_au': lambda p: 0.5 * (p['actionness'] + 1) * p['uncertainty'],
}


def results_json(result_dict, threshold=None, version="THUMOS14"):
    """The result-file layout AFSD/evaluation reads: {'version', 'results': {video: [proposal, ...]}, 'external_data'}."""
    ext = {} if threshold is None else {'threshold': float(threshold)}
    return {"version": version, "results": dict(result_dict), "external_data": ext}


def ood_threshold(result_dict, scoring='uncertainty'):
    """The known/unknown operating point of AFSD/thumos14/threshold.py:128-150: run the detector over the TRAINING
    videos, turn every detection into a known-ness score (1 - its OOD score) and take the value that 95 % of the
    detections exceed."""
    import numpy as np
    score = OOD_SCORES[scoring]
    all_scores = [1 - score(p) for props in result_dict.values() for p in props]
    n = len(all_scores)
    if n == 0:
        raise ValueError("no detections to threshold")
    return float(np.sort(all_scores)[n - int(n * 0.95) - 1])


# ----------------------------------------------------------------------------- what the drivers share (test.py:59-64, :203-288)
def prepare_data(data_path, video_name, crop_size, device='cuda'):
    """test.py:59-64: <video>.npy uint8 (T,H,W,3) -> centre-cropped planar (3,T,crop,crop) uint8 on the device."""
    import os
    import numpy as np
    data = np.load(os.path.join(data_path, video_name + '.npy'))
    data = np.transpose(data, [3, 0, 1, 2])
    h, w = data.shape[2:]
    i, j = int(np.round((h - crop_size) / 2.)), int(np.round((w - crop_size) / 2.))
    return torch.from_numpy(np.ascontiguousarray(data[:, :, i:i + crop_size, j:j + crop_size])).to(device)


def gather_results(result_dict, names, rank, world, device=None):
    """Several ranks (video list sharded): every rank's result dict travels to rank 0, which returns the merged
    dict in the video list's order (the pattern sketched in AFSD/anet/test.py:248-273, with a collective instead of
    multiprocessing queues); the other ranks return None.  One rank: the dict itself."""
    if world == 1:
        return result_dict
    import torch.distributed as dist
    if not dist.is_initialized():
        import os
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29534')
        if device is not None and torch.device(device).type == 'cuda':
            dist.init_process_group(backend='nccl', rank=rank, world_size=world, device_id=torch.device(device))
        else:
            dist.init_process_group(backend='gloo', rank=rank, world_size=world)
    parts = [None] * world if rank == 0 else None
    dist.gather_object(result_dict, parts, dst=0)
    if rank != 0:
        return None
    merged = {}
    for part in parts:
        merged.update(part)
    return {n: merged[n] for n in names if n in merged}

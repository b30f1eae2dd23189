"""MultiSegmentLoss of OpenTAL/AFSD (reference AFSD/thumos14/multisegment_loss.py:70-259) with the
same constructor and the same 7-tuple result, vectorised over the batch and free of host
synchronisation: anchor<->GT matching runs for all clips at once on padded targets, and every
"select the positives, then reduce" of the reference is a masked reduction over all anchors.

The loss ablations of the paper (configs/ablations/thumos14_opental_{focal,ghm,ib,hardmib,noMIB,noIoUC,noACT}.yaml) differ from
the final recipe only in model.os_head and training.edl_config; all seven run through the single-launch loss (otal_detection_loss_ex
for the focal / ghm / ib re-weightings and for noACT = closed-set EDL with IBM).  So do the other standard EDL settings,
edl_config.evidence relu / softplus and loss_type digamma / mse (otal_detection_loss_ev, csrc/evidence.h); only mse with a
re-weighting rule or IBM configured keeps the torch formulation (the reference's mse_loss ignores the rules, and the kernel
refuses the combination).

os_head=False is the closed-set variant of the Softmax and EDL baselines (configs thumos14_softmax.yaml,
thumos14_open_edl.yaml): C = classes + 1 logits with class 0 = background, EVERY anchor is classified against its matched
label, and there are no actionness terms (loss_act, loss_prop_act are None, multisegment_loss.py:196-231, :250-255).
cls_loss_type='rpl' (thumos14_open_rpl.yaml, thumos14_open_gcpl.yaml; closed-set only): conf / prop_conf are the distances of
RPLHead and the two classification terms are cls_loss.RPLoss (multisegment_loss.py:201-204, :225-228).

Reference quirks kept on purpose (documented in DESIGN.md):
  * the IoU-calibration term pairs iou_pred (stored prior-major, (126,B)) with logits flattened
    batch-major (multisegment_loss.py:116,:234-236) -- identical for batch 1, the yaml's batch size;
  * the tIoU target of the quality head carries gradient into loc / prop_loc (it is not detached,
    multisegment_loss.py:176-187);
  * 'rpl': the refined stage asks RPLoss for the MEAN over the anchors (reduction=True, :228) and still divides by PN (:248).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..common.input_pipeline import PaddedTargets
from .cls_loss import REWEIGHT, ActionnessLoss, EvidenceLoss, FocalLoss_Ori, RPLoss

_EPS = torch.finfo(torch.float32).eps
FUSED = True      # single-launch HIP loss for the final recipe and the closed-set baselines (set False to force the torch formulation)


def _tiou(pred, target):
    inter = torch.min(pred[..., 0], target[..., 0]) + torch.min(pred[..., 1], target[..., 1])
    union = (target[..., 0] + target[..., 1]) + (pred[..., 0] + pred[..., 1]) - inter
    return inter / union.clamp(min=_EPS), inter, union


def iou_loss(pred, target, weight=None, loss_type='giou', reduction='none'):
    """(multisegment_loss.py:20-53); any leading shape, last dim = (left, right) extents."""
    ious, _, union = _tiou(pred, target)
    if loss_type == 'linear_iou':
        loss = 1.0 - ious
    elif loss_type == 'giou':
        hull = torch.max(pred[..., 0], target[..., 0]) + torch.max(pred[..., 1], target[..., 1])
        loss = 1.0 - (ious - (hull - union) / hull.clamp(min=_EPS))
    else:
        loss = ious
    if weight is not None:
        loss = loss * weight.view(loss.size())
    if reduction == 'sum':
        return loss.sum()
    if reduction == 'mean':
        return loss.mean()
    return loss


_PAD_INDEX = {}     # (target counts, device) -> (row index of every target in the padded (B*G) table, validity mask); device tensors


def pad_targets(targets, device):
    """list of (n_i,3) [start,end,label] -> (B,G,3) padded + (B,G) validity, built from host shapes.
    Three launches whatever the batch (concatenate, zero, scatter the rows): the scatter index and the mask depend only on
    the per-sample target counts and are cached on the device.  A first-time count pattern met while a HIP graph is being
    captured takes the per-sample form (no host -> device copy may be recorded into the graph)."""
    lens = tuple(int(t.shape[0]) for t in targets)
    G, B = max(lens), len(targets)
    device = torch.device(device)
    key = (lens, device)
    hit = _PAD_INDEX.get(key)
    if hit is None and not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        if len(_PAD_INDEX) > 256:
            _PAD_INDEX.clear()
        idx = torch.tensor([i * G + j for i, n in enumerate(lens) for j in range(n)], dtype=torch.long).to(device)
        valid = (torch.arange(G).view(1, G) < torch.tensor(lens).view(B, 1)).to(device)
        hit = _PAD_INDEX[key] = (idx, valid)
    if hit is None:
        out = torch.zeros(B, G, 3, device=device)
        valid = torch.zeros(B, G, dtype=torch.bool, device=device)
        for i, t in enumerate(targets):
            out[i, :lens[i]] = t.to(device)
            valid[i, :lens[i]] = True
        return out, valid
    idx, valid = hit
    rows = torch.cat([t.to(device=device, dtype=torch.float32).reshape(-1, 3) for t in targets], 0)     # (sum n_i, 3)
    out = torch.zeros(B * G, 3, device=device).index_copy_(0, idx, rows).view(B, G, 3)
    return out, valid


def as_padded(targets, device):
    """(rows (B,G,3), validity (B,G)) of either form of a batch's targets: the reference's list of ragged (n_i,3) arrays
    (padded here to the batch's longest list) or an input_pipeline.PaddedTargets (fixed G, used as it is)."""
    if isinstance(targets, PaddedTargets):
        return targets.gt, targets.valid
    if isinstance(targets, (list, tuple)):
        return pad_targets(targets, device)
    return targets


def kernel_focal_alpha0(focal):
    """The focal_alpha of the HIP loss kernels for a FocalLoss_Ori -- its alpha of class 0 -- when it has their form (gamma 2,
    one alpha for every other class, the two summing to 1), else None.  Read at construction, while alpha is on the host."""
    al = focal.alpha
    if focal.gamma == 2 and al.numel() >= 2 and bool((al[1:] == al[1]).all()) and abs(float(al[0]) + float(al[1]) - 1.0) < 1e-6:
        return float(al[0])
    return None


class MultiSegmentLoss(nn.Module):
    def __init__(self, num_classes, overlap_thresh, negpos_ratio, use_gpu=True, cls_loss_type='focal',
                 edl_config=None, rpl_config=None, os_head=False, act_config=None, size_average=False,
                 clip_length=256):
        super(MultiSegmentLoss, self).__init__()
        self.num_classes = num_classes
        self.overlap_thresh = overlap_thresh
        self.negpos_ratio = negpos_ratio
        self.use_gpu = use_gpu
        self.cls_loss_type = cls_loss_type
        self.clip_length = clip_length      # config['dataset']['training']['clip_length'] (:110)
        self._focal_alpha0 = None
        if cls_loss_type == 'focal':
            self.cls_loss = FocalLoss_Ori(num_classes, balance_index=0, size_average=size_average, alpha=0.25)
            self._focal_alpha0 = kernel_focal_alpha0(self.cls_loss)
        elif cls_loss_type == 'edl':
            self.cls_loss = EvidenceLoss(num_classes, edl_config, size_average=size_average)
        elif cls_loss_type == 'rpl':
            if rpl_config is None:
                raise NotImplementedError("cls_loss_type 'rpl' needs the rpl_config of the RPL / GCPL yaml")
            if os_head:
                raise NotImplementedError("cls_loss_type 'rpl' with os_head: the distance head is closed-set only")
            self.cls_loss = RPLoss(num_classes, rpl_config, size_average=size_average)
        else:
            raise NotImplementedError(f"cls_loss_type {cls_loss_type!r}")
        self.iou_aware = cls_loss_type == 'edl' and self.cls_loss.iou_aware
        self.os_head = os_head
        # the closed-set variant has no actionness heads (multisegment_loss.py:87-88)
        self.act_loss = ActionnessLoss(size_average=size_average, cfg=act_config) if os_head else None
        self.size_average = size_average

    @torch.no_grad()
    def match(self, loc, priors, targets):
        """Anchor <-> GT assignment for the whole batch (multisegment_loss.py:120-153)."""
        clip = float(self.clip_length)
        gt, valid = as_padded(targets, loc.device)
        valid = valid.bool()
        c = priors[:, 0].view(1, -1, 1)                                     # (1,K,1)
        left = (c - gt[:, None, :, 0]) * clip                               # (B,K,G)
        right = (gt[:, None, :, 1] - c) * clip
        big = clip * 2
        area = left + right
        area = torch.where((left < 0) | (right < 0) | ~valid[:, None, :], torch.full_like(area, big), area)
        best_area, best = area.min(-1)                                      # first minimum, like torch.min
        g0 = torch.gather(gt[:, :, 0], 1, best)
        g1 = torch.gather(gt[:, :, 1], 1, best)
        lab = torch.gather(gt[:, :, 2], 1, best)
        p = priors[:, 0].view(1, -1)
        loc_t = torch.stack([(p - g0) * clip, (g1 - p) * clip], -1)
        conf_t = torch.where(best_area >= big, torch.zeros_like(lab), lab).long()
        iou = _tiou(loc, loc_t)[0]
        prop_conf_t = torch.where(iou < self.overlap_thresh, torch.zeros_like(conf_t), conf_t)
        w = (loc[..., 0] + loc[..., 1]).unsqueeze(-1)
        prop_loc_t = (loc_t - loc) / (0.5 * w)
        return loc_t, conf_t, prop_loc_t, prop_conf_t, iou

    def _fused_ok(self, loc):
        """The single-launch HIP loss (csrc/loss.hip) covers the final recipe and the closed-set baselines; other settings
        use the torch formulation."""
        return self._cls_mode(loc) is not None

    def fused_route(self):
        """Which HIP entry of csrc/loss.hip this criterion's SETTINGS select at its current epoch -- no tensors are read -- or
        None where the torch formulation below runs.  -> (entry, cls_mode, kinds, reweight, ibm_active):
          entry     'plain' (otal_detection_loss), 'ex' (otal_detection_loss_ex: a re-weighting rule in force, or IBM active
                    over a closed set), 'ev' (otal_detection_loss_ev: any evidence / loss_type but exp / log) or 'rpl'
                    (otal_detection_loss_rpl);
          cls_mode  0 = EDL with actionness (OpenTAL), 1 = focal with actionness (as-shipped dispatch), 2 = closed-set EDL (with
                    IBM it is the noACT ablation), 3 = closed-set focal; 'rpl' with the entry of that name;
          kinds     None unless 'ev', then (evidence, loss_type) numbered as csrc/evidence.h: _kinds();
          reweight  cls_loss.REWEIGHT of the rule EvidenceLoss.reweight() picks at this epoch (with_focal / with_ghm / with_ibloss);
          ibm_active  that rule is the influence-balanced weight.
        'mse' with a re-weighting rule or IBM configured is not the kernel's (the reference's mse_loss ignores them): None."""
        from ..common.ops import EVIDENCE, LOSS_TYPE
        cl = self.cls_loss
        if not FUSED or self.size_average or cl.size_average:
            return None
        if self.os_head and (self.act_loss.weight != 0 or self.act_loss.size_average):
            return None
        if self.cls_loss_type == 'rpl':
            return ('rpl', 'rpl', None, 0, False) if float(cl.temp) > 0 else None
        if self.cls_loss_type == 'focal':       # the as-shipped THUMOS14 dispatch (train.py:27-31) / thumos14_softmax.yaml
            return ('plain', 1 if self.os_head else 3, None, 0, False) if self._focal_alpha0 is not None else None
        if self.cls_loss_type != 'edl' or cl.num_bins > 64 or cl.evidence not in EVIDENCE or cl.loss_type not in LOSS_TYPE:
            return None
        if cl.loss_type == 'mse' and (cl.with_focal or cl.with_ghm or cl.with_ibloss or cl.with_ibm):
            return None
        mode = 0 if self.os_head else 2
        rule = cl.reweight()
        ibm, rw = rule == 'ibm', REWEIGHT[rule]
        kinds = self._kinds()
        if kinds != (0, 0):
            return 'ev', mode, kinds, rw, ibm
        # a re-weighting rule of the loss ablations, or IBM over a closed set (noACT): the extended entry
        return 'ex' if rw != 0 or (mode == 2 and ibm) else 'plain', mode, None, rw, ibm

    def _route(self, loc):
        """fused_route() where `loc` is what the kernel takes (a float32 device tensor of at most 2048 anchors), else None."""
        if not (loc.is_cuda and loc.dtype == torch.float32 and loc.shape[0] * loc.shape[1] <= 2048):
            return None
        return self.fused_route()

    def _cls_mode(self, loc):
        """cls_mode of fused_route() for this tensor, or None where the torch formulation below runs."""
        route = self._route(loc)
        return None if route is None else route[1]

    def _kinds(self):
        """(evidence, loss_type) of otal_detection_loss_ev for this criterion's EvidenceLoss."""
        from ..common.ops import EVIDENCE, LOSS_TYPE
        return EVIDENCE[self.cls_loss.evidence], LOSS_TYPE[self.cls_loss.loss_type]

    def _loss_call(self, route, device):
        """(ops.LossCall, state) of the launch `route` names: the host scalars of the entry, and the tensor the kernel reads and
        updates -- the GHM populations or the IBM EMA; one unused float where the mode has neither, None for 'rpl'."""
        from ..common.ops import LossCall
        entry, mode, kinds, rw, ibm = route
        cl = self.cls_loss
        own = dict(entry=entry, clip_length=float(self.clip_length), overlap_thresh=float(self.overlap_thresh))
        if mode == 'rpl':
            return LossCall(gcpl=bool(cl.gcpl), temperature=float(cl.temp), weight_pl=float(cl.weight_pl), radius=float(cl.radius),
                            **own), None
        if mode in (1, 3):                      # focal: no EMA, no rule, no IoU calibration
            if getattr(self, '_no_ibm', None) is None or self._no_ibm.device != device:
                self._no_ibm = torch.ones(1, dtype=torch.float32, device=device)     # unused EMA slot of the ABI
            return LossCall(cls_mode=mode, focal_alpha=self._focal_alpha0, **own), self._no_ibm
        evidence, loss_type = kinds or (0, 0)
        # (the closed-set mode passes its momentum only with a rule or IBM in force: nothing else reads it)
        momentum = float(cl.momentum) if (mode == 0 or ibm or rw) else 0.0
        call = LossCall(cls_mode=mode, focal_alpha=float(cl.focal_alpha), ibm_active=ibm, iou_aware=bool(self.iou_aware),
                        evidence=evidence, loss_type=loss_type, num_bins=cl.num_bins, momentum=momentum, reweight=rw,
                        rw_gamma=float(cl.gamma), **own)
        return call, cl.acc_sum if rw == REWEIGHT['ghm'] else cl.weight_accum

    def forward(self, output_dict, targets, pre_locs=None):
        loc, conf = output_dict['loc'], output_dict['conf']
        prop_loc, prop_conf = output_dict['prop_loc'], output_dict['prop_conf']
        center, priors = output_dict['center'], output_dict['priors']
        act, prop_act = output_dict.get('act'), output_dict.get('prop_act')
        B, K = loc.shape[0], priors.shape[0]
        C = self.num_classes
        route = self._route(loc)
        if route is not None:
            from ..common import ops
            gt, valid = as_padded(targets, loc.device)
            call, state = self._loss_call(route, loc.device)
            if route[1] == 'rpl':
                fn, acts = ops.RPLDetectionLossFunction, ()
            else:
                fn = ops.DetectionLossFunction
                acts = (act.reshape(B, K), prop_act.reshape(B, K)) if self.os_head else (None, None)
            out = fn.apply(loc, conf, prop_loc, prop_conf, center.reshape(B, K), *acts, priors[:, 0], gt, valid, state, call)
            return out if self.os_head else out[:5] + (None, None)
        loc_t, conf_t, prop_loc_t, prop_conf_t, iou_pred = self.match(loc.detach(), priors, targets)
        pos, prop_pos = conf_t > 0, prop_conf_t > 0
        zero = loc.new_zeros(())
        # coarse localisation: GIoU over positives
        loss_l = torch.where(pos, iou_loss(loc, loc_t, loss_type='giou'), zero).sum()
        # refined localisation: L1 over refined positives
        loss_prop_l = torch.where(prop_pos.unsqueeze(-1), (prop_loc - prop_loc_t).abs(), zero).sum()
        # quality head: BCE(center, tIoU of the refined segment); the target is NOT detached
        w = (loc[..., 0] + loc[..., 1]).unsqueeze(-1)
        cur = 0.5 * w * prop_loc + loc
        q = _tiou(cur, loc_t)[0].clamp(min=0)
        x = center.view(B, K)
        bce = torch.clamp(x, min=0) - x * q + torch.log1p(torch.exp(-x.abs()))
        loss_ct = torch.where(pos, bce, zero).sum()

        def classify(logits, tgt, refined=False):
            lg = logits.reshape(-1, C)
            t = tgt.reshape(-1)
            keep = t > 0
            if not self.os_head:                # closed set: every anchor, its matched label (0 = background)
                if self.cls_loss_type == 'rpl':
                    return self.cls_loss(lg, t, reduction=refined), keep
                if self.cls_loss_type == 'focal':
                    return self.cls_loss(F.softmax(lg, dim=1), t), keep
                return self.cls_loss(lg, t), keep
            cls_id = (t - 1).clamp(min=0)
            if self.cls_loss_type == 'focal':
                return self.cls_loss(F.softmax(lg, dim=1), cls_id, keep), keep
            return self.cls_loss(lg, cls_id, keep), keep

        loss_c, keep = classify(conf, conf_t)
        loss_prop_c, pkeep = classify(prop_conf, prop_conf_t, refined=True)
        loss_act = loss_prop_act = None
        if self.os_head:
            loss_act, AN = self.act_loss(act.reshape(-1, 1), keep.to(act.dtype))
            loss_prop_act, PAN = self.act_loss(prop_act.reshape(-1, 1), pkeep.to(act.dtype))
        N = pos.sum().clamp(min=1)
        PN = prop_pos.sum().clamp(min=1)
        if not self.size_average:
            loss_l, loss_c, loss_ct = loss_l / N, loss_c / N, loss_ct / N
            loss_prop_l, loss_prop_c = loss_prop_l / PN, loss_prop_c / PN
            if self.os_head:
                loss_act, loss_prop_act = loss_act / AN, loss_prop_act / PAN
        if self.iou_aware:
            # reference pairing: iou_pred is (K,B) flattened prior-major against batch-major logits
            ious = iou_pred.transpose(0, 1).reshape(-1)
            loss_prop_c = loss_prop_c + self.cls_loss.iou_calib(prop_conf.reshape(-1, C), ious, mean=True)
        return loss_l, loss_c, loss_prop_l, loss_prop_c, loss_ct, loss_act, loss_prop_act

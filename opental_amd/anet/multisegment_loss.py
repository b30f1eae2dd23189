"""MultiSegmentLoss of the ActivityNet1.3 recipe (reference AFSD/anet/multisegment_loss.py:87-301): same constructor,
same `predictions` list and the same 7-tuple.  The reference loops over the samples of the batch in Python and
normalises every term per sample before averaging; here all samples are matched and reduced at once on padded
targets with masked per-sample reductions -- no host synchronisation.

What differs from the THUMOS14 loss and is reproduced: per-level regression bounds on max(left, right) (:69-84,
:156-166); refined-stage positives use min(overlap_thresh, best IoU among the sample's positives) (:178-184);
smooth-L1 for the refinement (:206); IoU calibration pairs each sample's logits with its own IoUs (:259-261).

os_head=False is the closed-set variant of the Softmax and EDL baselines (configs anet_softmax.yaml, anet_edl.yaml):
C = 151 logits with class 0 = background, EVERY anchor is classified against its matched label (0 where unmatched), and
there are no actionness terms (loss_act, loss_prop_act are None, :226-257, :282-286).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..thumos14.multisegment_loss import _tiou, as_padded, iou_loss, kernel_focal_alpha0, pad_targets  # noqa: F401  (iou_loss: reference name)
from .cls_loss import ActionnessLoss, EvidenceLoss, FocalLoss_Ori

bounds = [[0, 30], [15, 60], [30, 120], [60, 240], [96, 768], [256, 768]]
FUSED = True      # one workgroup per sample (csrc/loss.hip) for the EDL and focal settings; False forces the torch formulation


class MultiSegmentLoss(nn.Module):
    def __init__(self, num_classes, overlap_thresh, negpos_ratio, use_gpu=True, cls_loss_type='focal', edl_config=None,
                 os_head=False, size_average=False, clip_length=768):
        super(MultiSegmentLoss, self).__init__()
        self.num_classes = num_classes
        self.overlap_thresh = overlap_thresh
        self.negpos_ratio = negpos_ratio
        self.use_gpu = use_gpu
        self.cls_loss_type = cls_loss_type
        self.clip_length = clip_length          # config['dataset']['training']['clip_length'] (:118)
        if size_average:
            raise NotImplementedError("size_average: the reference's `x /= N if not size_average else x` divides a "
                                      "loss by itself in that mode; the recipe never sets it")
        self._focal_alpha0 = None
        if cls_loss_type == 'focal':
            self.cls_loss = FocalLoss_Ori(num_classes, balance_index=0, size_average=False, alpha=0.25)
            self._focal_alpha0 = kernel_focal_alpha0(self.cls_loss)
        elif cls_loss_type == 'edl':
            self.cls_loss = EvidenceLoss(num_classes, edl_config, size_average=False)
        else:
            raise NotImplementedError(cls_loss_type)
        self.iou_aware = cls_loss_type == 'edl' and self.cls_loss.iou_aware
        self.os_head = os_head
        # the closed-set variant has no actionness heads (:101-102)
        self.act_loss = ActionnessLoss(size_average=False, weight=0.1) if os_head else None
        self.size_average = size_average
        self.register_buffer('level_bounds', torch.tensor(bounds, dtype=torch.float32), persistent=False)

    @torch.no_grad()
    def match(self, loc, priors, targets):
        """Anchor <-> GT assignment for the whole batch (anet/multisegment_loss.py:144-188)."""
        clip = float(self.clip_length)
        gt, valid = as_padded(targets, loc.device)
        valid = valid.bool()
        lvl = priors[:, 1].long()
        lb = self.level_bounds.to(loc.device)[lvl, 0].view(1, -1, 1)
        rb = self.level_bounds.to(loc.device)[lvl, 1].view(1, -1, 1)
        c = priors[:, 0].view(1, -1, 1)                                     # (1,K,1)
        left = (c - gt[:, None, :, 0]) * clip                               # (B,K,G)
        right = (gt[:, None, :, 1] - c) * clip
        far = torch.max(left, right)
        big = clip * 2
        area = left + right
        out = (left < 0) | (right < 0) | (far <= lb) | (far > rb) | ~valid[:, None, :]
        area = torch.where(out, torch.full_like(area, big), area)
        best_area, best = area.min(-1)                                      # first minimum, like torch.min
        g0 = torch.gather(gt[:, :, 0], 1, best)
        g1 = torch.gather(gt[:, :, 1], 1, best)
        lab = torch.gather(gt[:, :, 2], 1, best)
        p = priors[:, 0].view(1, -1)
        loc_t = torch.stack([(p - g0) * clip, (g1 - p) * clip], -1)
        conf_t = torch.where(best_area >= big, torch.zeros_like(lab), lab).long()
        iou = _tiou(loc, loc_t)[0]
        pos = conf_t > 0
        best_iou = iou.masked_fill(~pos, -float('inf')).max(-1)[0]
        thr = torch.where(pos.any(-1), best_iou.clamp(max=float(self.overlap_thresh)),
                          torch.full_like(best_iou, float(self.overlap_thresh)))
        prop_conf_t = torch.where(iou < thr.unsqueeze(-1), torch.zeros_like(conf_t), conf_t)
        w = (loc[..., 0] + loc[..., 1]).unsqueeze(-1)
        prop_loc_t = (loc_t - loc) / (0.5 * w)
        return loc_t, conf_t, prop_loc_t, prop_conf_t, iou

    def _bounds_list(self):
        """The level table of the `level_bounds` BUFFER (the single source of truth of both paths), as host floats."""
        lb = self.level_bounds
        key = (lb.data_ptr(), lb._version)
        if getattr(self, '_bounds_key', None) != key:
            self._bounds_host, self._bounds_key = lb.detach().cpu().tolist(), key
        return self._bounds_host

    def _fused_ok(self, loc, conf, priors):
        return self._cls_mode(loc, conf, priors) is not None

    def fused_route(self):
        """Which HIP entry of this recipe (csrc/loss.hip) this criterion's SETTINGS select -- no tensors are read -- or None
        where the torch formulation below runs.  -> (entry, cls_mode, kinds, ibm_active):
          entry     'anet_ex' (otal_detection_loss_anet_ex: what the three shipped configs launch) or 'anet_ev'
                    (otal_detection_loss_anet_ev);
          cls_mode  0 = EDL with actionness (configs/anet_opental.yaml), 2 = closed-set EDL (anet_edl.yaml), 3 = closed-set
                    focal (anet_softmax.yaml);
          kinds     None with 'anet_ex', else (evidence, loss_type) numbered as csrc/evidence.h;
          ibm_active  the influence-balanced weight at the criterion's current epoch.
        (exp, log) goes to 'anet_ex' unless it is closed-set with IBM configured, which that entry refuses; every other pair goes
        to 'anet_ev'.  The reference's mse_loss applies no weight, and the kernel refuses mse with IBM: an mse config that has
        `with_ibm` keeps the torch formulation (which ignores the flag, as the reference does)."""
        from ..common.ops import EVIDENCE, LOSS_TYPE
        cl = self.cls_loss
        if not FUSED or cl.size_average or self.size_average:
            return None
        if self.cls_loss_type == 'focal':
            if self.os_head or self._focal_alpha0 is None:
                return None
            return 'anet_ex', 3, None, False
        if self.cls_loss_type != 'edl' or cl.evidence not in EVIDENCE or cl.loss_type not in LOSS_TYPE:
            return None
        if self.os_head and self.act_loss.size_average:
            return None
        if cl.loss_type == 'mse' and cl.with_ibm:
            return None
        mode = 0 if self.os_head else 2
        ibm = bool(cl.with_ibm and cl.epoch >= cl.ibm_start)
        if (cl.evidence, cl.loss_type) == ('exp', 'log') and (self.os_head or not cl.with_ibm):
            return 'anet_ex', mode, None, ibm
        return 'anet_ev', mode, (EVIDENCE[cl.evidence], LOSS_TYPE[cl.loss_type]), ibm

    def _route(self, loc, conf, priors):
        """fused_route() where the tensors are what the kernel takes, else None."""
        cl = self.cls_loss
        if not (FUSED and loc.is_cuda and loc.dtype == torch.float32 and priors.shape[0] <= 1024 and priors.shape[1] == 2
                and conf.shape[-1] == self.num_classes and self.num_classes < 32768 and not cl.size_average
                and self.level_bounds.shape[0] <= 8):        # (the kernel keeps labels in 16 bits and <= MAX_LEVELS_A = 8 levels)
            return None
        route = self.fused_route()
        if route is None:
            return None
        # the kernel clamps a prior's level id into the table; the torch path would raise on an out-of-range one: keep the
        # torch path's behaviour for such priors (checked once per priors tensor -- one host read, not one per step)
        key = (priors.data_ptr(), priors._version, tuple(priors.shape))
        if getattr(self, '_lvl_checked', None) != key:
            self._lvl_ok = bool(0 <= int(priors[:, 1].min()) and int(priors[:, 1].max()) < self.level_bounds.shape[0])
            self._lvl_checked = key
        return route if self._lvl_ok else None

    def _cls_mode(self, loc, conf, priors):
        """cls_mode of fused_route() for these tensors, or None where the torch formulation below runs."""
        route = self._route(loc, conf, priors)
        return None if route is None else route[1]

    def _loss_call(self, route):
        """The host scalars (ops.LossCall) of the launch `route` names."""
        from ..common.ops import LossCall
        entry, mode, kinds, ibm = route
        evidence, loss_type = kinds or (0, 0)
        # (what an entry's mode does not read is passed as 0: the IBM coefficient of the closed-set modes of 'anet_ex', the
        # actionness settings without actionness heads)
        return LossCall(entry=entry, clip_length=float(self.clip_length), overlap_thresh=float(self.overlap_thresh), cls_mode=mode,
                        focal_alpha=self._focal_alpha0 if mode == 3 else 0.25, ibm_active=ibm, iou_aware=bool(self.iou_aware),
                        evidence=evidence, loss_type=loss_type, level_bounds=self._bounds_list(),
                        ibm_coeff=float(self.cls_loss.coeff) if (mode == 0 or entry == 'anet_ev') else 0.0,
                        act_weight=float(self.act_loss.weight) if self.os_head else 0.0,
                        act_margin=float(self.act_loss.margin) if self.os_head else 0.0)

    def forward(self, predictions, targets, pre_locs=None):
        loc, conf, prop_loc, prop_conf, center, priors, act, prop_act = predictions
        B, K = loc.shape[0], priors.shape[0]
        route = self._route(loc, conf, priors)
        if route is not None:
            from ..common.ops import AnetDetectionLossFunction
            gt, valid = as_padded(targets, loc.device)
            acts = (act.reshape(B, K), prop_act.reshape(B, K)) if self.os_head else (None, None)
            out = AnetDetectionLossFunction.apply(loc, conf, prop_loc, prop_conf, center.reshape(B, K), *acts, priors, gt, valid,
                                                  None, self._loss_call(route))
            return out if self.os_head else out[:5] + (None, None)
        loc_t, conf_t, prop_loc_t, prop_conf_t, iou_pred = self.match(loc.detach(), priors, targets)
        pos, prop_pos = conf_t > 0, prop_conf_t > 0
        zero = loc.new_zeros(())
        loss_l = torch.where(pos, iou_loss(loc, loc_t, loss_type='giou'), zero).sum(-1)
        d = (prop_loc - prop_loc_t).abs()
        sl1 = torch.where(d < 1.0, 0.5 * d * d, d - 0.5)
        loss_prop_l = torch.where(prop_pos.unsqueeze(-1), sl1, zero).sum((-1, -2))
        # quality head: BCE(center, tIoU of the refined segment); the target is NOT detached (:212-222)
        w = (loc[..., 0] + loc[..., 1]).unsqueeze(-1)
        cur = 0.5 * w * prop_loc + loc
        q = _tiou(cur, loc_t)[0].clamp(min=0)
        x = center.view(B, K)
        bce = torch.clamp(x, min=0) - x * q + torch.log1p(torch.exp(-x.abs()))
        loss_ct = torch.where(pos, bce, zero).sum(-1)

        def classify(logits, tgt):
            keep = tgt > 0
            if self.os_head:
                cls_id, mask = (tgt - 1).clamp(min=0), keep
            else:                               # closed set: every anchor, its matched label (0 = background)
                cls_id, mask = tgt, torch.ones_like(keep)
            if self.cls_loss_type == 'focal':
                return self.cls_loss(F.softmax(logits, dim=-1), cls_id, mask), keep
            return self.cls_loss(logits, cls_id, mask), keep

        loss_c, keep = classify(conf, conf_t)
        loss_prop_c, pkeep = classify(prop_conf, prop_conf_t)
        N = pos.sum(-1).clamp(min=1)
        PN = prop_pos.sum(-1).clamp(min=1)
        loss_l, loss_c, loss_ct = loss_l / N, loss_c / N, loss_ct / N
        loss_prop_l, loss_prop_c = loss_prop_l / PN, loss_prop_c / PN
        if self.iou_aware:
            loss_prop_c = loss_prop_c + self.cls_loss.iou_calib(prop_conf, iou_pred, mean=True)
        if not self.os_head:
            return tuple(v.sum() / B for v in (loss_l, loss_c, loss_prop_l, loss_prop_c, loss_ct)) + (None, None)
        loss_act, AN = self.act_loss(act.view(B, K), keep.to(act.dtype))
        loss_prop_act, PAN = self.act_loss(prop_act.view(B, K), pkeep.to(act.dtype))
        loss_act, loss_prop_act = loss_act / AN, loss_prop_act / PAN
        return tuple(v.sum() / B for v in (loss_l, loss_c, loss_prop_l, loss_prop_c, loss_ct, loss_act, loss_prop_act))

"""Classification / actionness losses of OpenTAL with the reference's class names and constructor
arguments (AFSD/thumos14/cls_loss.py: FocalLoss_Ori :6-78, EvidenceLoss :81-285, ActionnessLoss
:288-339, RPLoss :342-378), re-expressed for the GPU: every function takes ALL anchors plus a boolean mask and
uses masked sums, scatter-adds and rank masks, so there is no boolean-mask gather, no `.item()`
and no Python loop over bins -- i.e. no host synchronisation inside the training step
(the reference syncs ~60 times per step in these losses).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _evidence(logit, kind='exp'):
    if kind == 'exp':
        return torch.exp(torch.clamp(logit, -10, 10))
    if kind == 'relu':
        return F.relu(logit)
    if kind == 'softplus':
        return F.softplus(logit)
    raise NotImplementedError(kind)


class FocalLoss_Ori(nn.Module):
    """-alpha_c (1 - p)^gamma log(p + 1e-6) on softmax probabilities (cls_loss.py:6-78)."""

    def __init__(self, num_class, alpha=None, gamma=2, balance_index=-1, size_average=True):
        super(FocalLoss_Ori, self).__init__()
        self.num_class, self.gamma, self.size_average, self.eps = num_class, gamma, size_average, 1e-6
        if alpha is None:
            alpha = [0.25, 0.75]
        if isinstance(alpha, (list, tuple)):
            assert len(alpha) == num_class
            a = torch.Tensor(list(alpha))
        elif isinstance(alpha, (float, int)):
            assert 0 < alpha < 1.0 and balance_index > -1
            a = torch.ones(num_class) * (1 - alpha)
            a[balance_index] = alpha
        else:
            a = alpha
        self.register_buffer('alpha', a, persistent=False)

    def forward(self, prob, target, mask=None):
        """prob (N,K) softmax scores, target (N,) class ids, mask (N,) rows that count."""
        target = target.view(-1)
        pt = prob.gather(1, target.view(-1, 1)).view(-1) + self.eps
        loss = -torch.pow(1.0 - pt, self.gamma) * (self.alpha.to(prob.device)[target] * pt.log())
        if mask is not None:
            loss = torch.where(mask, loss, torch.zeros_like(loss))
            return loss.sum() / mask.sum().clamp(min=1) if self.size_average else loss.sum()
        return loss.mean() if self.size_average else loss.sum()


REWEIGHT = {None: 0, 'ibm': 0, 'focal': 1, 'ghm': 2, 'ib': 3}     # `reweight` of otal_detection_loss_ex (IBM is its ibm_active)


class EvidenceLoss(nn.Module):
    """EDL loss ('log' / 'digamma' / 'mse', evidence exp / relu / softplus) with influence-balanced (IBM) re-weighting from
    a 50-bin EMA (cls_loss.py:186-285) and the IoU-calibration term (cls_loss.py:120-129), and the three re-weightings of the
    loss ablations for 'log' / 'digamma' (cls_loss.py:221-256): focal-EDL, GHM and the closed-form influence-balanced loss.
    Every evidence / loss_type combination runs inside the single-launch HIP loss (csrc/loss.hip, arithmetic in
    csrc/evidence.h) except 'mse' with a re-weighting rule or IBM configured; this masked torch formulation is the host form
    of the same rule and what the kernels are tested against."""

    def __init__(self, num_cls, cfg, size_average=False):
        super(EvidenceLoss, self).__init__()
        self.num_cls = num_cls
        self.loss_type = cfg['loss_type']
        self.evidence = cfg['evidence']
        if self.loss_type not in ('log', 'digamma', 'mse'):
            raise NotImplementedError(self.loss_type)
        if cfg.get('soft_label', 0.0):
            raise NotImplementedError("soft_label")
        self.iou_aware = cfg.get('iou_aware', False)
        # the loss ablations (configs/ablations/thumos14_opental_{focal,ghm,ib}.yaml; cls_loss.py:94-108): one re-weighting
        # rule applies per call, in the order of the reference's elif chain -- see reweight()
        self.with_focal = cfg.get('with_focal', False)
        self.with_ghm = cfg.get('with_ghm', False)
        self.with_ibloss = cfg.get('with_ibloss', False)
        self.with_ibm = cfg.get('with_ibm', False)
        self.ibm_start = cfg.get('ibm_start', 0)
        self.ghm_start = cfg.get('ghm_start', 0)
        self.ib_start = cfg.get('ib_start', 10)
        self.num_bins = cfg.get('num_bins', 50)
        self.momentum = cfg.get('momentum', 0.99)
        self.gamma = cfg['gamma'] if self.with_focal else 0.0
        self.focal_alpha = cfg['alpha'] if self.with_focal else 0.25
        if self.with_focal:
            a = torch.ones(num_cls) * (1 - cfg['alpha'])
            a[0] = cfg['alpha']         # class id 0: the background of a closed set, the FIRST ACTION under os_head (ids are label - 1)
            self.register_buffer('alpha_class', a, persistent=False)
        # checkpointed here (the reference forgets to save it)
        self.register_buffer('weight_accum', torch.ones(self.num_bins))
        if self.with_ghm:
            # the GHM bin populations (an EMA when momentum > 0), carried from call to call; a buffer of the ghm configs only,
            # so every other criterion's state dict keeps its keys
            self.register_buffer('acc_sum', torch.zeros(self.num_bins))
            e = [float(x) / self.num_bins for x in range(self.num_bins + 1)]
            e[-1] += 1e-6
            self.register_buffer('edges', torch.tensor(e, dtype=torch.float32), persistent=False)
        self.epoch, self.total_epoch = 0, 25
        self.size_average = size_average

    def evidence_func(self, logit):
        return _evidence(logit, self.evidence)

    def iou_calib(self, logits, ious, mean=False):
        ious = torch.where(ious < 0, torch.full_like(ious, 1e-3), ious)
        u = self.num_cls / (self.evidence_func(logits) + 1).sum(dim=-1)
        reg = -ious * torch.log(1 - u) - (1 - ious) * torch.log(u)
        return reg.mean() if mean else reg.sum()

    def reweight(self):
        """The re-weighting rule of this call, by the reference's elif chain (cls_loss.py:221-272): 'focal' (ungated), 'ghm'
        (epoch >= ghm_start), 'ib' (epoch >= ib_start), 'ibm' (epoch >= ibm_start) or None.  The number otal_detection_loss_ex
        takes is REWEIGHT[rule]."""
        if self.with_focal:
            return 'focal'
        if self.with_ghm and self.epoch >= self.ghm_start:
            return 'ghm'
        if self.with_ibloss and self.epoch >= self.ib_start:
            return 'ib'
        if self.with_ibm and self.epoch >= self.ibm_start:
            return 'ibm'
        return None

    def state(self):
        """The tensor this criterion carries from step to step (None without one): the IBM EMA or the GHM bin populations."""
        if self.with_ghm and not self.with_focal:
            return self.acc_sum
        return self.weight_accum if self.with_ibm else None

    def forward(self, logit, target, mask=None):
        """logit (N,K), target (N,) in [0,K) (any valid id where mask is False), mask (N,) bool."""
        target = target.view(-1)
        if mask is None:
            mask = torch.ones_like(target, dtype=torch.bool)
        alpha = self.evidence_func(logit) + 1
        S = alpha.sum(dim=1, keepdim=True)
        if self.loss_type == 'mse':
            # mse_loss + loglikelihood_loss (cls_loss.py:186-201,:280-285): squared error of the Dirichlet mean plus its
            # variance, summed over the positives; the IBM / focal re-weightings do not apply to this loss type there either
            y = F.one_hot(target, self.num_cls).to(alpha.dtype)
            per = ((y - alpha / S) ** 2).sum(1) + (alpha * (S - alpha) / (S * S * (S + 1))).sum(1)
            per = torch.where(mask, per, torch.zeros_like(per))
            return per.sum() / mask.sum().clamp(min=1) if self.size_average else per.sum()
        func = torch.log if self.loss_type == 'log' else torch.digamma
        a_y = alpha.gather(1, target.view(-1, 1))
        per = (func(S) - func(a_y)).view(-1)          # sum_k y_k (f(S) - f(alpha_k)) with one-hot y
        rule = self.reweight()
        if rule == 'focal':
            # alpha_y (1 - max_k alpha_k / S)^gamma, NOT detached (cls_loss.py:224-227): the weight carries gradient
            score = (alpha / S).max(1)[0]
            per = self.alpha_class[target] * torch.pow(1.0 - score, self.gamma) * per
        elif rule == 'ghm':
            with torch.no_grad():
                g = torch.abs(1 / a_y.view(-1) - self.num_cls / S.view(-1))
                m = mask.to(g.dtype)
                inbin = ((g.unsqueeze(1) >= self.edges[:-1]) & (g.unsqueeze(1) < self.edges[1:])).to(g.dtype)    # (N, bins)
                cnt = (inbin * m.unsqueeze(1)).sum(0)
                # the reference bins every element of |1/alpha - u| * y: the zeros of the C - 1 other columns of each of the
                # M counted rows fall into bin 0 (cls_loss.py:232-237)
                cnt[0] += m.sum() * (self.num_cls - 1)
                valid = cnt > 0
                if self.momentum > 0:
                    self.acc_sum.copy_(torch.where(valid, self.momentum * self.acc_sum + (1 - self.momentum) * cnt, self.acc_sum))
                    pop = self.acc_sum
                else:
                    pop = cnt
                wbin = torch.where(valid, 1.0 / pop.clamp(min=1e-30), torch.zeros_like(pop))
                w = (inbin * wbin).sum(1) / valid.sum().clamp(min=1)
            per = w * per
        elif rule == 'ib':
            with torch.no_grad():
                g = torch.abs(1 / a_y.view(-1) - self.num_cls / S.view(-1))
                w = 1 / (g * logit.abs().sum(1))                # no epsilon, as the reference (cls_loss.py:254)
                w = torch.where(mask, w, torch.zeros_like(w))   # (a row that does not count must not send 0 * inf backwards)
            per = w * per
        elif rule == 'ibm':
            with torch.no_grad():
                u = self.num_cls / S.view(-1)
                gnorm = torch.abs(1 / a_y.view(-1) - u)
                ghat = gnorm * logit.abs().sum(1)
                bins = torch.ceil(gnorm * self.num_bins).long()                 # 1..num_bins (0 if gnorm == 0)
                slot = torch.remainder(bins - 1, self.num_bins)                 # python-style [-1] of the reference
                m = mask.to(ghat.dtype)
                tot = torch.zeros(self.num_bins, device=logit.device).index_add_(0, slot, ghat * m)
                cnt = torch.zeros(self.num_bins, device=logit.device).index_add_(0, slot, m)
                # the reference only updates bins 1..num_bins; bin 0 reads slot -1 without updating it
                upd_cnt = torch.zeros(self.num_bins, device=logit.device).index_add_(0, slot, m * (bins > 0).to(m.dtype))
                upd_tot = torch.zeros(self.num_bins, device=logit.device).index_add_(0, slot, ghat * m * (bins > 0).to(m.dtype))
                new = self.momentum * self.weight_accum + (1 - self.momentum) * upd_tot / upd_cnt.clamp(min=1)
                self.weight_accum.copy_(torch.where(upd_cnt > 0, new, self.weight_accum))
                w = self.weight_accum[slot]
            per = w * per
        per = torch.where(mask, per, torch.zeros_like(per))
        return per.sum() / mask.sum().clamp(min=1) if self.size_average else per.sum()


class ActionnessLoss(nn.Module):
    """Positive-unlabelled BCE: positives + the top-M lowest-scoring negatives, M = min(P, N) - 1
    (cls_loss.py:288-339).  Returns (loss, number of samples used) -- both tensors, no sync."""

    def __init__(self, size_average=False, cfg=None):
        super(ActionnessLoss, self).__init__()
        self.size_average = size_average
        self.weight = cfg.get('weight', 0.1) if cfg is not None else 0.1
        self.margin = cfg.get('margin', 1.0) if cfg is not None else 1.0

    def forward(self, logit, target):
        pred = logit.reshape(-1)
        pos = target.reshape(-1) > 0
        neg = ~pos
        npos, nneg = pos.sum(), neg.sum()
        top_m = torch.minimum(npos, nneg) - 1
        big = torch.finfo(pred.dtype).max
        order = torch.argsort(torch.where(neg, pred.detach(), torch.full_like(pred, big)))
        rank = torch.empty_like(order).scatter_(0, order, torch.arange(order.numel(), device=order.device))
        use_neg = torch.where(top_m > 0, neg & (rank < top_m), neg)
        used = pos | use_neg
        bce = F.binary_cross_entropy_with_logits(pred, pos.to(pred.dtype), reduction='none')
        bce = torch.where(used, bce, torch.zeros_like(bce))
        count = used.sum()
        loss = bce.sum() / count.clamp(min=1) if self.size_average else bce.sum()
        if self.weight != 0:
            neg_max = torch.where(neg, pred, torch.full_like(pred, -big)).max()
            pos_max = torch.where(pos, pred, torch.full_like(pred, -big)).max().detach()
            rank_loss = torch.clamp(self.margin - neg_max + pos_max, min=0.0)
            loss = loss + self.weight * torch.where(top_m > 0, rank_loss, torch.zeros_like(rank_loss))
        return loss, count


class RPLoss(nn.Module):
    """The classification term of the RPL and GCPL baselines (cls_loss.py:342-378) on the distances of RPLHead:
    softmax cross-entropy on dist / T (RPL: far from the reciprocal points) or -dist / T (GCPL: near the prototypes), plus
    a regulariser on the distance to the label's own centre.  Written in terms of dist and d_i = dist[i, y_i]: the
    reference's (feats - centers[labels]).pow(2).mean(1) IS d_i, so `feats` and `centers` are accepted for the reference's
    signature and not read -- their gradient flows through dist.
      RPL   CE + weight_pl * mse(d, radius), both with the call's reduction ('sum'; 'mean' with reduction=True)
      GCPL  CE + weight_pl * mean(d) / 2 -- F.mse_loss(feats, centers[labels]) / 2 is a mean over A * D whatever the reduction
    `radius` is a one-element parameter of the reference's criterion that no optimizer ever holds (train.py:321 passes
    net.parameters() only): it stays 0, and is a plain attribute here."""

    def __init__(self, num_classes, cfg, size_average=False):
        super(RPLoss, self).__init__()
        self.weight_pl = cfg['weight_pl'] if 'weight_pl' in cfg else 0.1
        self.temp = cfg['temperature'] if 'temperature' in cfg else 1
        self.gcpl = cfg['gcpl'] if 'gcpl' in cfg else False
        self.radius = 0.0
        self.size_average = size_average
        self.num_cls = num_classes

    def forward(self, dist, targets, feats=None, centers=None, reduction=False):
        mean = self.size_average or reduction
        labels = targets.view(-1)
        d = dist.gather(1, labels.view(-1, 1)).squeeze(1)
        if self.gcpl:
            loss = F.cross_entropy(-dist / self.temp, labels, reduction='mean' if mean else 'sum')
            return loss + self.weight_pl * (d.mean() / 2)
        loss = F.cross_entropy(dist / self.temp, labels, reduction='mean' if mean else 'sum')
        e = (d - self.radius) ** 2
        return loss + self.weight_pl * (e.mean() if mean else e.sum())

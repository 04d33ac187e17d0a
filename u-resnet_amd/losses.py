"""The loss of the device loss head (csrc/loss_head.hip), stated once.

Per voxel p: logits z, q = softmax(z), C classes, l = int(label[p]) truncated toward zero, w = weight[p] (1 without a weight),
P = n * voxels:

    t_k    = (1 - smoothing) [k == l] + smoothing / C
    ce_p   = -sum_k t_k log q_k                 f_p = (1 - q_l)^gamma      (1 at gamma == 0)
    L_ce   = (1/n) sum_p w_p f_p ce_p           sum over voxels, mean over events: the reference's reduction (lib/ssnet.py:57-71)
    I_c    = sum_p q_pc [l_p == c]   S_c = sum_p q_pc   Y_c = sum_p [l_p == c]        all P voxels of the batch, unweighted
    D_c    = (2 I_c + dice_eps) / (S_c + Y_c + dice_eps)
    L_dice = 1 - (1/C) sum_c D_c                L = L_ce + dice_weight * L_dice

A voxel with l == ignore_label adds nothing to L_ce, the Dice sums or dL/dz, but still counts in the accuracies.  Any other label
outside [0, C) makes the loss NaN, as in the plan's head.

``loss_numpy`` is the fp64 oracle with the analytic gradient written out; ``loss_torch`` states the same definition through torch
autograd for ``accum_gradients_custom``.
"""
import math

import numpy as np


class LossSpec(object):
    """gamma: focal exponent, 0 or >= 1 (the derivative of (1 - p)^gamma is unbounded at p -> 1 for 0 < gamma < 1, so that range
    is refused); smoothing in [0, 1); dice_weight >= 0; dice_eps > 0; ignore_label an integer (-1: none)."""
    __slots__ = ('gamma', 'smoothing', 'dice_weight', 'dice_eps', 'ignore_label')

    def __init__(self, gamma=0.0, smoothing=0.0, dice_weight=0.0, dice_eps=1.0, ignore_label=-1):
        gamma, smoothing, dice_weight, dice_eps = float(gamma), float(smoothing), float(dice_weight), float(dice_eps)
        if not math.isfinite(gamma) or not (gamma == 0.0 or gamma >= 1.0):
            raise ValueError('LossSpec: gamma = %r must be 0 or >= 1 and finite' % gamma)
        if not (0.0 <= smoothing < 1.0):
            raise ValueError('LossSpec: smoothing = %r outside [0, 1)' % smoothing)
        if not math.isfinite(dice_weight) or dice_weight < 0.0:
            raise ValueError('LossSpec: dice_weight = %r is negative or not finite' % dice_weight)
        if not math.isfinite(dice_eps) or dice_eps <= 0.0:
            raise ValueError('LossSpec: dice_eps = %r is not a positive finite number' % dice_eps)
        if isinstance(ignore_label, bool) or not isinstance(ignore_label, (int, np.integer)):
            raise ValueError('LossSpec: ignore_label = %r is not an integer' % (ignore_label,))
        if not -2 ** 31 <= int(ignore_label) < 2 ** 31:
            raise ValueError('LossSpec: ignore_label = %r does not fit 32 bits' % (ignore_label,))
        object.__setattr__(self, 'gamma', gamma)
        object.__setattr__(self, 'smoothing', smoothing)
        object.__setattr__(self, 'dice_weight', dice_weight)
        object.__setattr__(self, 'dice_eps', dice_eps)
        object.__setattr__(self, 'ignore_label', int(ignore_label))

    def __setattr__(self, name, value):
        raise AttributeError('LossSpec is immutable')

    @property
    def neutral(self):
        """True when the loss is the reference's weighted cross-entropy: the kernel then takes the heads' own statements."""
        return self.gamma == 0.0 and self.smoothing == 0.0 and self.dice_weight == 0.0 and self.ignore_label == -1

    @property
    def active(self):
        return not self.neutral

    def __repr__(self):
        return 'LossSpec(gamma=%g, smoothing=%g, dice_weight=%g, dice_eps=%g, ignore_label=%d)' % (
            self.gamma, self.smoothing, self.dice_weight, self.dice_eps, self.ignore_label)


def loss_numpy(logits, data, label, weight, spec):
    """fp64.  logits [n, ..., C]; data (nullable) / label / weight (nullable) [n, ...].  Returns a dict: loss, ce_term, dice_term,
    acc_all, acc_nonzero (NaN without data or without a voxel with data > 0) and dlogits (shape of logits): the analytic
    d loss / d logits."""
    z = np.asarray(logits, dtype=np.float64)
    n, C = z.shape[0], z.shape[-1]
    z = z.reshape(n, -1, C)
    V = z.shape[1]
    lab = np.trunc(np.asarray(label, dtype=np.float64).reshape(n, V)).astype(np.int64)
    w = np.ones((n, V)) if weight is None else np.asarray(weight, dtype=np.float64).reshape(n, V)
    m = z.max(-1, keepdims=True)
    e = np.exp(z - m)
    ssum = e.sum(-1, keepdims=True)
    q = e / ssum
    logq = (z - m) - np.log(ssum)
    ign = (lab == spec.ignore_label) if spec.ignore_label != -1 else np.zeros((n, V), bool)
    ok = (lab >= 0) & (lab < C)
    hit = ok & ~ign
    bad = ~ok & ~ign
    labc = np.where(ok, lab, 0)
    onehot = (np.arange(C)[None, None, :] == labc[..., None]).astype(np.float64)
    s = spec.smoothing
    # 1 - q_l from the other classes' terms: exact where q_l rounds to 1; likewise -log q_l = log1p(others / e_l)
    eo, el = (e * (1.0 - onehot)).sum(-1), (e * onehot).sum(-1)
    om = eo / ssum[..., 0]
    ql = (q * onehot).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        cel = np.where(eo < 0.5 * el, np.log1p(eo / np.where(el > 0, el, 1.0)), -(onehot * logq).sum(-1))
    ce = (1.0 - s) * cel - (s / C) * logq.sum(-1)
    g = spec.gamma
    if g == 0.0:
        f, fm1 = np.ones((n, V)), np.zeros((n, V))
    else:
        with np.errstate(divide='ignore', invalid='ignore'):
            fm1 = np.ones((n, V)) if g == 1.0 else np.where(om > 0, om ** (g - 1.0), 0.0)
        f = fm1 * om
    live = (~ign).astype(np.float64)
    ce_sum = (w * f * ce * live).sum()
    ce_term = ce_sum / n
    if bad.any():
        ce_term = float('nan')
    # d ce_k = f (q_k - t_k) - gamma (1 - q_l)^(gamma - 1) q_l ([k == l] - q_k) ce
    q_minus_1hot = np.where(onehot > 0, -om[..., None], q)
    dce = f[..., None] * (q_minus_1hot + s * (onehot - 1.0 / C)) - (g * fm1 * ql * ce)[..., None] * (-q_minus_1hot)
    dl = (w * live / n)[..., None] * dce
    dice_term = 0.0
    if spec.dice_weight > 0.0:
        hot = onehot * hit[..., None]
        ql_ = q * live[..., None]
        I, S, Y = (ql_ * hot).sum((0, 1)), ql_.sum((0, 1)), hot.sum((0, 1))
        U = S + Y + spec.dice_eps
        D = (2.0 * I + spec.dice_eps) / U
        dice_term = 1.0 - D.mean()
        a = -2.0 / (C * U)
        b = (2.0 * I + spec.dice_eps) / (C * U * U)
        r = a[None, None, :] * hot + b[None, None, :]
        dl = dl + spec.dice_weight * live[..., None] * q * (r - (q * r).sum(-1, keepdims=True))
    loss = ce_term + spec.dice_weight * dice_term
    pred = z.argmax(-1)   # lowest index on ties, as the strict '>' of the heads
    okp = pred == lab
    acc_all = okp.mean()
    acc_nonzero = float('nan')
    if data is not None:
        nz = np.asarray(data, dtype=np.float64).reshape(n, V) > 0
        if nz.any():
            acc_nonzero = (okp & nz).sum() / nz.sum()
    return {'loss': float(loss), 'ce_term': float(ce_term), 'dice_term': float(dice_term), 'acc_all': float(acc_all),
            'acc_nonzero': float(acc_nonzero), 'dlogits': dl.reshape(np.asarray(logits).shape)}


def loss_torch(spec, label, weight=None):
    """``loss_fn(logits)`` for ``accum_gradients_custom``: the same definition through torch autograd (logits
    [n, ..., C], any float dtype, any device; label / weight [n, ...] arrays or tensors).  An independent statement of the
    gradient: nothing of ``loss_numpy``'s analytic form is used."""
    import torch

    def loss_fn(logits):
        n, C = logits.shape[0], logits.shape[-1]
        z = logits.reshape(n, -1, C)
        V = z.shape[1]
        lab = torch.as_tensor(label).to(device=z.device).reshape(n, V).to(torch.float64).trunc().to(torch.int64)
        w = torch.ones((n, V), dtype=z.dtype, device=z.device) if weight is None else \
            torch.as_tensor(weight).to(device=z.device, dtype=z.dtype).reshape(n, V)
        ign = (lab == spec.ignore_label) if spec.ignore_label != -1 else torch.zeros_like(lab, dtype=torch.bool)
        ok = (lab >= 0) & (lab < C)
        live = (~ign).to(z.dtype)
        onehot = torch.nn.functional.one_hot(torch.where(ok, lab, torch.zeros_like(lab)), C).to(z.dtype)
        logq = torch.log_softmax(z, dim=-1)
        q = logq.exp()
        t = (1.0 - spec.smoothing) * onehot + spec.smoothing / C
        ce = -(t * logq).sum(-1)
        if spec.gamma == 0.0:
            f = torch.ones_like(ce)
        else:
            om = (q * (1.0 - onehot)).sum(-1)   # 1 - q_l
            f = om ** spec.gamma
        ce_term = (w * f * ce * live).sum() / n
        if bool((~ok & ~ign).any()):
            ce_term = ce_term * float('nan')
        loss = ce_term
        if spec.dice_weight > 0.0:
            hot = onehot * (ok & ~ign).to(z.dtype)[..., None]
            ql = q * live[..., None]
            I, S, Y = (ql * hot).sum((0, 1)), ql.sum((0, 1)), hot.sum((0, 1))
            D = (2.0 * I + spec.dice_eps) / (S + Y + spec.dice_eps)
            loss = loss + spec.dice_weight * (1.0 - D.mean())
        return loss

    return loss_fn

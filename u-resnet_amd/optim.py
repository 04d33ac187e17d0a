"""The guarded optimiser step in numpy: what ``ursn_opt_stats`` / ``ursn_opt_decide`` / ``ursn_opt_adam`` (include/uresnet_hip.h,
opt_guard.hip) compute, stated without the device's summation order, and the learning-rate schedule of the driver.

Not in the reference, whose optimiser is a bare ``tf.train.AdamOptimizer().apply_gradients`` over the summed minibatch gradients
(lib/ssnet.py:72-80): no look at the gradient, no clipping, no weight decay, no schedule.

* statistics: per tensor ``sum g^2`` and ``sum p^2`` in float64 over the FINITE elements, ``max |g|`` over them, and the number of
  non-finite ``g`` (NaN, +-Inf), which contribute 0 and are only counted; globally the sum over tensors, its square root, the
  total count;
* decision: ``coef = float32(clip_norm / norm)`` (one float64 division, rounded once) when ``clip_norm > 0`` and
  ``norm > clip_norm``, else 1; ``skip = skip_nonfinite and nonfinite > 0``;
* update: nothing on skip; else ``g' = g * coef`` in float32, ``p' = p * float32(1 - lr * weight_decay)`` for the tensors that decay
  (decoupled AdamW, rounded to float32 before the update), then Adam in TensorFlow's form with every operation rounded on its own.
  The step counter ``t`` advances on every guarded call, skipped or not: the host cannot know a skip without a synchronisation.
"""
from __future__ import print_function

import numpy as np

BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8


def _segments(g, p, infos):
    """``(name, g_segment, p_segment or None)`` per tensor.  ``g`` / ``p``: dicts name -> array (``get_gradients()`` /
    ``get_variables()``; ``infos`` unused), or flat arrays with ``infos`` a sequence of ``(name, offset, nelem)``."""
    if isinstance(g, dict):
        for name, a in g.items():
            yield name, np.asarray(a, np.float32).reshape(-1), (None if p is None else np.asarray(p[name], np.float32).reshape(-1))
        return
    g = np.asarray(g, np.float32).reshape(-1)
    p = None if p is None else np.asarray(p, np.float32).reshape(-1)
    for info in infos:
        name, off, n = info[0], int(info[1]), int(info[2])
        yield name, g[off:off + n], (None if p is None else p[off:off + n])


def _sumsq(x):
    x = x.astype(np.float64)
    return float(np.sum(x * x))


def grad_stats_numpy(g, p=None, infos=None):
    """Dict keyed by tensor name with ``grad_sumsq``, ``grad_norm``, ``grad_maxabs``, ``nonfinite``, ``param_sumsq``, ``param_norm``
    (the last two 0.0 without ``p``), plus ``'global'``: ``grad_sumsq`` (tensors added in order), ``grad_norm``, ``nonfinite``."""
    out, total, bad = {}, 0.0, 0
    for name, gs, ps in _segments(g, p, infos):
        fin = np.isfinite(gs)
        gf = np.where(fin, gs, np.float32(0))
        ss = _sumsq(gf)
        psq = 0.0
        if ps is not None:
            psq = _sumsq(np.where(np.isfinite(ps), ps, np.float32(0)))
        nf = int(gs.size - np.count_nonzero(fin))
        out[name] = {'grad_sumsq': ss, 'grad_norm': float(np.sqrt(ss)), 'grad_maxabs': float(np.max(np.abs(gf))) if gf.size else 0.0,
                     'nonfinite': nf, 'param_sumsq': psq, 'param_norm': float(np.sqrt(psq))}
        total += ss
        bad += nf
    out['global'] = {'grad_sumsq': total, 'grad_norm': float(np.sqrt(total)), 'nonfinite': bad}
    return out


def clip_coef_numpy(norm, clip_norm):
    """The float32 factor the gradient is multiplied by."""
    clip = float(np.float32(clip_norm))
    norm = float(norm)
    if clip > 0.0 and norm > clip:
        return np.float32(clip / norm)
    return np.float32(1.0)


def lr_t_numpy(lr, t):
    """Adam's bias-corrected step size as the library's host code forms it: float64, rounded to float32 once."""
    lr = float(np.float32(lr))
    return np.float32(lr * np.sqrt(1.0 - BETA2 ** float(t)) / (1.0 - BETA1 ** float(t)))


def adam_numpy(p, g, m, v, lr, t):
    """One plain Adam step (TF form) on float32 arrays, every operation rounded to float32 on its own; returns (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    b1, b2, eps, lr_t = f(BETA1), f(BETA2), f(EPSILON), lr_t_numpy(lr, t)
    m2 = b1 * m + (f(1) - b1) * g
    v2 = b2 * v + (f(1) - b2) * g * g
    return p - lr_t * m2 / (np.sqrt(v2) + eps), m2, v2


def guarded_adam_numpy(p, g, m, v, infos, t, lr, clip_norm=0.0, weight_decay=0.0, skip_nonfinite=False):
    """One guarded step on flat float32 arrays.  ``infos``: ``(name, offset, nelem, decay_flag)`` per tensor; elements outside every
    tensor are left alone.  Returns ``(p, m, v, status)``, ``status`` = dict ``sumsq`` / ``norm`` / ``nonfinite`` / ``coef`` / ``skip``."""
    f = np.float32
    p, g, m, v = (np.array(a, f).reshape(-1) for a in (p, g, m, v))
    glob = grad_stats_numpy(g, None, infos)['global']
    coef = clip_coef_numpy(glob['grad_norm'], clip_norm)
    skip = bool(skip_nonfinite) and glob['nonfinite'] > 0
    status = {'sumsq': glob['grad_sumsq'], 'norm': glob['grad_norm'], 'nonfinite': glob['nonfinite'], 'coef': coef, 'skip': int(skip)}
    if skip:
        return p, m, v, status
    decay = f(1.0 - float(f(lr)) * float(f(weight_decay)))
    with np.errstate(all='ignore'):
        for info in infos:
            off, n = int(info[1]), int(info[2])
            s = slice(off, off + n)
            ps = p[s] * decay if info[3] else p[s]
            p[s], m[s], v[s] = adam_numpy(ps, g[s] * coef, m[s], v[s], lr, t)
    return p, m, v, status


def lr_at(cfg, iteration):
    """The driver's learning rate at ``iteration`` (0-based), a pure function of it so that a resumed run repeats the schedule:
    ``base = LEARNING_RATE`` (0.001, AdamOptimizer's default, when it is <= 0); for ``iteration < LR_WARMUP_STEPS`` the linear ramp
    ``base * (iteration + 1) / LR_WARMUP_STEPS``, which starts at ``base / LR_WARMUP_STEPS`` and reaches ``base`` on the last warm-up
    step; afterwards ``base * LR_DECAY_RATE ** (iteration // LR_DECAY_STEPS)`` (``LR_DECAY_STEPS`` 0: no decay).  With the three keys
    at their defaults it is ``base`` itself."""
    base = cfg.LEARNING_RATE if (cfg.LEARNING_RATE is not None and cfg.LEARNING_RATE > 0) else 0.001
    it = int(iteration)
    warm, steps = int(cfg.LR_WARMUP_STEPS), int(cfg.LR_DECAY_STEPS)
    if warm > 0 and it < warm:
        return base * (it + 1) / float(warm)
    if steps > 0:
        return base * float(cfg.LR_DECAY_RATE) ** (it // steps)
    return base


def schedule_on(cfg):
    return int(cfg.LR_WARMUP_STEPS) > 0 or (int(cfg.LR_DECAY_STEPS) > 0 and float(cfg.LR_DECAY_RATE) != 1.0)

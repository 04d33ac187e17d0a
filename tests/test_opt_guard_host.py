"""Host side of the guarded optimiser step (no device): the numpy definitions of optim.py against straightforward loops, the
learning-rate schedule, the driver keys, the refusals of the op-level entries that come before any device access
(include/uresnet_hip.h, "guarded optimiser step"), and the order of all-reduce and statistics inside apply_gradients."""
import ctypes
import math
import os

import numpy as np
import pytest

from uresnet_amd import _lib, optim, ssnet_config, uresnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ursn_opt_state_size", "ursn_opt_state_layout", "ursn_opt_state_init", "ursn_opt_stats", "ursn_opt_decide", "ursn_opt_adam",
       "ursn_opt_state_read", "ursn_opt_state_bytes", "ursn_opt_attach", "ursn_grad_stats", "ursn_apply_adam_guarded", "ursn_opt_read")


def test_new_symbols_are_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "uresnet_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in hdr, name
    assert lib.ursn_abi_version() == 9
    assert "#define URSN_OPT_CHUNK 4096" in hdr
    assert ctypes.sizeof(_lib.ursn_opt_status) == 48 and ctypes.sizeof(_lib.ursn_opt_tensor) == 32
    assert ctypes.sizeof(_lib.ursn_opt_desc) == 16


# ---- numpy definitions against loops ----------------------------------------------------------------------------------------
INFOS = [("a", 0, 5, 1), ("b", 7, 1, 0), ("c", 8, 9, 1)]      # elements 5, 6 belong to no tensor


def _flat(seed, n=17, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def _loop_stats(g, p, infos):
    out, total, bad = {}, 0.0, 0
    for name, off, n in [i[:3] for i in infos]:
        ss = ps = 0.0
        mx, nf = 0.0, 0
        for k in range(off, off + n):
            x = float(g[k])
            if math.isnan(x) or math.isinf(x):
                nf += 1
            else:
                ss += x * x
                mx = max(mx, abs(x))
            if p is not None and math.isfinite(float(p[k])):
                ps += float(p[k]) * float(p[k])
        out[name] = (ss, mx, nf, ps)
        total += ss
        bad += nf
    return out, total, bad


def test_grad_stats_numpy_against_loops_and_counts_nonfinite():
    g, p = _flat(1), _flat(2)
    g[2], g[7], g[10], g[6] = np.nan, np.inf, -np.inf, np.nan        # g[6] lies in no tensor: neither counted nor summed
    want, total, bad = _loop_stats(g, p, INFOS)
    got = optim.grad_stats_numpy(g, p, INFOS)
    assert bad == 3 and got['global']['nonfinite'] == 3
    assert [got[k]['nonfinite'] for k in "abc"] == [1, 1, 1]
    for k in "abc":
        ss, mx, nf, ps = want[k]
        assert got[k]['grad_sumsq'] == pytest.approx(ss, rel=1e-15) and got[k]['param_sumsq'] == pytest.approx(ps, rel=1e-15)
        assert got[k]['grad_maxabs'] == mx and got[k]['grad_norm'] == math.sqrt(got[k]['grad_sumsq'])
    assert got['b']['grad_sumsq'] == 0.0 and got['b']['grad_maxabs'] == 0.0        # its only element is +Inf
    assert math.isfinite(got['global']['grad_norm']) and got['global']['grad_sumsq'] == pytest.approx(total, rel=1e-15)
    # the dict form (get_gradients() / get_variables()) is the same statement
    gd = {n: g[o:o + k].reshape(-1, 1) for n, o, k, _ in INFOS}
    pd = {n: p[o:o + k].reshape(-1, 1) for n, o, k, _ in INFOS}
    assert optim.grad_stats_numpy(gd, pd) == got
    assert optim.grad_stats_numpy(g, None, INFOS)['a']['param_norm'] == 0.0


def test_clip_coef_numpy():
    f = np.float32
    assert optim.clip_coef_numpy(10.0, 0.0) == f(1) and optim.clip_coef_numpy(10.0, -1.0) == f(1)
    assert optim.clip_coef_numpy(10.0, 10.0) == f(1) and optim.clip_coef_numpy(3.0, 10.0) == f(1)
    c = optim.clip_coef_numpy(7.0, 3.0)
    assert c.dtype == np.float32 and c == f(3.0 / 7.0)
    assert optim.clip_coef_numpy(7.0, f(0.1)) == f(float(f(0.1)) / 7.0)              # the clip is the float32 the desc carries


def _loop_guarded(p, g, m, v, infos, t, lr, clip, wd, skip_nf):
    f = np.float32
    p, m, v = p.copy(), m.copy(), v.copy()
    _, total, bad = _loop_stats(g, None, infos)
    norm = math.sqrt(total)
    coef = f(float(f(clip)) / norm) if clip > 0 and norm > float(f(clip)) else f(1)
    if skip_nf and bad:
        return p, m, v, coef, 1
    lr_t = f(float(f(lr)) * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    decay = f(1.0 - float(f(lr)) * float(f(wd)))
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    for _, off, n, flag in infos:
        for k in range(off, off + n):
            gk = f(g[k] * coef)
            pk = f(p[k] * decay) if flag else p[k]
            m[k] = f(f(b1 * m[k]) + f(f(f(1) - b1) * gk))
            v[k] = f(f(b2 * v[k]) + f(f(f(f(1) - b2) * gk) * gk))
            p[k] = f(pk - f(f(lr_t * m[k]) / f(np.sqrt(v[k]) + eps)))
    return p, m, v, coef, 0


@pytest.mark.parametrize("clip, wd, t", [(0.0, 0.0, 1), (0.5, 0.0, 1), (0.0, 0.1, 7), (0.5, 0.1, 1000)])
def test_guarded_adam_numpy_against_loops(clip, wd, t):
    p, g, m, v = _flat(3), _flat(4), _flat(5, scale=0.1), np.abs(_flat(6, scale=0.01))
    got = optim.guarded_adam_numpy(p, g, m, v, INFOS, t, 1e-3, clip, wd, True)
    want = _loop_guarded(p, g, m, v, INFOS, t, 1e-3, clip, wd, True)
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert got[3]['coef'] == want[3] and got[3]['skip'] == 0
    assert (got[3]['coef'] < 1) == (clip > 0)
    assert np.array_equal(got[0][5:7], p[5:7]) and not np.array_equal(got[0][:5], p[:5])       # outside every tensor: untouched
    if clip == 0.0 and wd == 0.0:                                                               # neutral == plain Adam
        plain = optim.adam_numpy(p, g, m, v, 1e-3, t)
        for k, (_, off, n, _) in enumerate(INFOS):
            assert np.array_equal(got[0][off:off + n], plain[0][off:off + n])


def test_guarded_adam_numpy_skips_on_nonfinite_only_when_asked():
    p, g, m, v = _flat(3), _flat(4), _flat(5, scale=0.1), np.abs(_flat(6, scale=0.01))
    g[9] = np.nan
    q, m2, v2, st = optim.guarded_adam_numpy(p, g, m, v, INFOS, 1, 1e-3, 0.5, 0.1, True)
    assert st['skip'] == 1 and st['nonfinite'] == 1 and math.isfinite(st['norm'])
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in ((q, p), (m2, m), (v2, v)))
    g[9] = 0.25
    assert optim.guarded_adam_numpy(p, g, m, v, INFOS, 1, 1e-3, 0.5, 0.1, False)[3]['skip'] == 0


# ---- schedule -------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    c = ssnet_config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_lr_at():
    assert all(optim.lr_at(_cfg(LEARNING_RATE=0.01), it) == 0.01 for it in (0, 1, 5, 10 ** 6))       # keys off: the constant
    assert optim.lr_at(_cfg(), 3) == 0.001 and optim.lr_at(_cfg(LEARNING_RATE=0), 3) == 0.001       # AdamOptimizer() default
    assert not optim.schedule_on(_cfg()) and not optim.schedule_on(_cfg(LR_DECAY_STEPS=5))
    c = _cfg(LEARNING_RATE=0.01, LR_WARMUP_STEPS=4)
    assert optim.schedule_on(c)
    assert [optim.lr_at(c, it) for it in range(6)] == [0.01 * 1 / 4.0, 0.01 * 2 / 4.0, 0.01 * 3 / 4.0, 0.01, 0.01, 0.01]
    assert optim.lr_at(c, 0) == 0.01 / 4                                                             # starts at LEARNING_RATE / W
    c = _cfg(LEARNING_RATE=0.01, LR_DECAY_STEPS=10, LR_DECAY_RATE=0.5)
    assert optim.schedule_on(c)
    assert [optim.lr_at(c, it) for it in (0, 9, 10, 19, 20, 35)] == [0.01, 0.01, 0.005, 0.005, 0.0025, 0.00125]
    c = _cfg(LEARNING_RATE=0.01, LR_WARMUP_STEPS=4, LR_DECAY_STEPS=10, LR_DECAY_RATE=0.5)
    assert optim.lr_at(c, 3) == 0.01 and optim.lr_at(c, 9) == 0.01 and optim.lr_at(c, 10) == 0.005
    assert optim.lr_at(c, 12) == optim.lr_at(c, 12)                                                  # pure: a resumed run repeats it


# ---- driver keys ----------------------------------------------------------------------------------------------------------------
def test_config_keys_default_off_parse_and_refuse_wrong_types(tmp_path):
    c = ssnet_config()
    assert (c.CLIP_GRAD_NORM, c.WEIGHT_DECAY, c.SKIP_NONFINITE, c.GRAD_STATS) == (0., 0., False, False)
    assert (c.LR_WARMUP_STEPS, c.LR_DECAY_STEPS, c.LR_DECAY_RATE) == (0, 0, 1.)
    f = tmp_path / "a.cfg"
    f.write_text("CLIP_GRAD_NORM 2.5\nWEIGHT_DECAY 0.01\nSKIP_NONFINITE True\nGRAD_STATS True\nLR_WARMUP_STEPS 100\n"
                 "LR_DECAY_STEPS 1000\nLR_DECAY_RATE 0.5\n")
    c.override(str(f))
    assert (c.CLIP_GRAD_NORM, c.WEIGHT_DECAY, c.SKIP_NONFINITE, c.GRAD_STATS) == (2.5, 0.01, True, True)
    assert (c.LR_WARMUP_STEPS, c.LR_DECAY_STEPS, c.LR_DECAY_RATE) == (100, 1000, 0.5)
    for bad in ("CLIP_GRAD_NORM 1", "CLIP_GRAD_NORM '1.0'", "CLIP_GRAD_NORM -1.0", "WEIGHT_DECAY True", "WEIGHT_DECAY -0.1",
                "SKIP_NONFINITE 1", "GRAD_STATS 'yes'", "LR_WARMUP_STEPS 2.0", "LR_WARMUP_STEPS -1", "LR_DECAY_STEPS 1.5",
                "LR_DECAY_RATE 1", "LR_DECAY_RATE 0.0"):
        f.write_text(bad + "\n")
        with pytest.raises(TypeError):
            ssnet_config().override(str(f))


# ---- refusals before any device access ------------------------------------------------------------------------------------------
def test_op_level_refusals(lib):
    i64 = lambda *a: (ctypes.c_int64 * len(a))(*a)
    nel, off, dec = i64(1, 4096, 4097), i64(0, 1, 4097), (ctypes.c_int32 * 3)(0, 1, 1)
    assert lib.ursn_opt_state_size(nel, 3) == 64 + 64 + 3 * 32 + 4 * 32 + 3 * 32 + 4 * 16
    lay = i64(0, 0, 0, 0, 0, 0)
    assert lib.ursn_opt_state_layout(nel, 3, lay) == 0 and list(lay) == [512, 64, 128, 224, 4, 4096]
    assert lib.ursn_opt_state_size(nel, 0) == 0 and lib.ursn_opt_state_size(i64(1, 0), 2) == 0 and lib.ursn_opt_state_size(None, 1) == 0
    err = lambda: lib.ursn_last_error().decode()
    aligned = ctypes.c_void_p(1 << 20)                      # never dereferenced: every call below is refused first
    assert lib.ursn_opt_state_init(None, 512, off, nel, dec, 3) != 0 and "null state" in err()
    assert lib.ursn_opt_state_init(ctypes.c_void_p((1 << 20) + 8), 512, off, nel, dec, 3) != 0 and "16-byte aligned" in err()
    assert lib.ursn_opt_state_init(aligned, 511, off, nel, dec, 3) != 0 and "too small, 512 needed" in err()
    assert lib.ursn_opt_state_init(aligned, 512, i64(0, 0, 4097), nel, dec, 3) != 0 and "overlap" in err()
    assert lib.ursn_opt_state_init(aligned, 512, i64(-1, 1, 4097), nel, dec, 3) != 0 and "out of range" in err()
    assert lib.ursn_opt_state_init(aligned, 512, off, nel, None, 3) != 0 and "null" in err()
    d = _lib.ursn_opt_desc()
    d.lr = 1e-3
    assert lib.ursn_opt_stats(ctypes.c_void_p((1 << 20) + 4), aligned, None, None) != 0 and "16-byte aligned" in err()
    assert lib.ursn_opt_stats(aligned, None, None, None) != 0 and "null gradient" in err()
    assert lib.ursn_opt_stats(aligned, ctypes.c_void_p((1 << 20) + 2), None, None) != 0 and "4-byte aligned" in err()
    assert lib.ursn_opt_decide(aligned, None, None) != 0 and "null desc" in err()
    assert lib.ursn_opt_adam(aligned, aligned, aligned, aligned, aligned, 10, ctypes.byref(d), 0, None) != 0 and "t = 0" in err()
    assert lib.ursn_opt_adam(aligned, aligned, aligned, None, aligned, 10, ctypes.byref(d), 1, None) != 0 and "null p / g / m / v" in err()
    d.lr = 0.0
    assert lib.ursn_opt_decide(aligned, ctypes.byref(d), None) != 0 and "lr = 0" in err()
    d.lr, d.weight_decay = 0.5, 4.0
    assert lib.ursn_opt_adam(aligned, aligned, aligned, aligned, aligned, 10, ctypes.byref(d), 1, None) != 0 and "outside [0, 1]" in err()
    assert lib.ursn_apply_adam_guarded(None, ctypes.byref(d), None) != 0 and lib.ursn_grad_stats(None, 1, None) != 0
    assert lib.ursn_opt_attach(None, aligned, 512) != 0 and "null handle" in err()


def test_state_bytes_of_a_configuration(lib):
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(allocate=False)
    need = ctypes.c_int64(0)
    assert lib.ursn_opt_state_bytes(ctypes.byref(net._cfg), ctypes.byref(need)) == 0
    nel = [n for _, _, _, n in net._specs]
    chunks = sum((n + 4095) // 4096 for n in nel)
    assert need.value == 128 + 64 * len(nel) + 48 * chunks
    assert need.value == lib.ursn_opt_state_size((ctypes.c_int64 * len(nel))(*nel), len(nel))


# ---- python surface without a device --------------------------------------------------------------------------------------------
def _stub_net(calls):
    """A constructed-but-unallocated net whose device-touching pieces are replaced by recorders."""
    net = uresnet(dims=[32, 32, 1], num_class=3, base_num_outputs=4, num_strides=2)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-3, allocate=False)
    net._handle, net._max_batch = ctypes.c_void_p(1), 1
    net._ensure_handle = lambda batch: None
    net._stream = lambda sess: None
    net._opt_require_state = lambda: calls.append("require_state")
    net.allreduce_gradients = lambda: calls.append("allreduce_gradients")
    net.allreduce_bn_moving = lambda: calls.append("allreduce_bn_moving")
    return net


class _FakeLib(object):
    def __init__(self, calls):
        self.calls, self.desc, self.lr = calls, None, None

    def ursn_apply_adam(self, handle, lr, stream):
        self.calls.append("ursn_apply_adam")
        self.lr = lr
        return 0

    def ursn_apply_adam_guarded(self, handle, desc, stream):
        self.calls.append("ursn_apply_adam_guarded")
        d = desc._obj
        self.desc = (d.lr, d.clip_norm, d.weight_decay, d.skip_nonfinite)
        return 0


def test_apply_gradients_reduces_over_ranks_before_the_statistics(monkeypatch):
    calls = []
    fake = _FakeLib(calls)
    net = _stub_net(calls)
    frozen = uresnet(dims=[32, 32, 1], num_class=3, base_num_outputs=4, num_strides=2)
    frozen.construct(trainable=False, use_weight=True, allocate=False)
    monkeypatch.setattr(_lib, "load", lambda: fake)                     # after construct, which queries the real plan
    net.apply_gradients(None)                                           # nothing attached: the plain call, as before
    assert calls == ["allreduce_gradients", "allreduce_bn_moving", "ursn_apply_adam"] and fake.lr == pytest.approx(1e-3)
    del calls[:]
    net.set_optimizer()                                                 # everything off: still the plain call
    net.apply_gradients(None, lr=5e-4)
    assert calls == ["allreduce_gradients", "allreduce_bn_moving", "ursn_apply_adam"] and fake.lr == pytest.approx(5e-4)
    del calls[:]
    net.set_optimizer(clip_norm=2.0, weight_decay=0.01, skip_nonfinite=True)
    net.apply_gradients(None, lr=5e-4)
    assert calls == ["allreduce_gradients", "allreduce_bn_moving", "require_state", "ursn_apply_adam_guarded"]
    assert fake.desc == (np.float32(5e-4), 2.0, np.float32(0.01), 1) and net._last_lr == 5e-4
    for bad in (dict(clip_norm=-1.0), dict(clip_norm=float("nan")), dict(weight_decay=-0.1), dict(weight_decay=float("inf"))):
        with pytest.raises(ValueError):
            net.set_optimizer(**bad)
    with pytest.raises(RuntimeError):
        frozen.set_optimizer(clip_norm=1.0)

"""Guarded optimiser step on the device (include/uresnet_hip.h, "guarded optimiser step"; opt_guard.hip), from the kernels up to
the driver keys.

Op level: synthetic flat buffers, segment lengths 1, 3, 8, CHUNK - 1, CHUNK, CHUNK + 1, 3 CHUNK + 5 (and 2 CHUNK + 2) with gaps
that put some offsets off a 16-byte boundary, the whole buffer shifted by 0..3 floats.  Every output sits in guarded buffers
(tests/_abi.py::_Guarded) and every comparison of arrays is on bit patterns (same_bits).

The exact cases use gradients k / 32 and parameters k / 64 with integer |k| <= 64: every square is a multiple of 2^-12 below 4,
every partial sum of fewer than 2^30 of them is exact in fp64 in any order, so np.sum(x.astype(f64) ** 2) is the oracle without
knowing the device's summation order.

The device's fp64 sqrt: every status record read in this file is checked for norm == sqrt(sumsq) on the host, bit for bit
(_State.read); that is the evidence behind DESIGN.md's statement that it is correctly rounded."""
import ctypes
import json
import math
import re

import numpy as np
import pytest

from _abi import _Guarded, same_bits
from uresnet_amd import _lib, optim, uresnet
from uresnet_amd import synthetic_io as sio

pytestmark = pytest.mark.gpu

CHUNK = 4096          # URSN_OPT_CHUNK; test_layout_constants pins it
GUARD = 4096
LENS = [1, 3, 8, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 2 * CHUNK + 2]
GAPS = [1, 1, 2, 5, 3, 0, 2, 1]        # floats in front of each segment
DECAY = [0, 1, 0, 1, 1, 0, 1, 0]
LONGEST = 6
NAN64 = 0x7FF8000000000000
SHIFTS = [0, 1, 2, 3]


def _table(lens=LENS, gaps=GAPS):
    offs, at = [], 0
    for n, gap in zip(lens, gaps):
        at += gap
        offs.append(at)
        at += n
    return offs, at + 3


OFFS, TOTAL = _table()
assert {o % 4 for o in OFFS} == {0, 1, 2, 3}          # offsets on and off the 16-byte boundary
INFOS = [("t%d" % i, o, n, d) for i, (o, n, d) in enumerate(zip(OFFS, LENS, DECAY))]


def _i64(a):
    return (ctypes.c_int64 * len(a))(*[int(x) for x in a])


class _Buf(object):
    """A host fp32 array on the device, `shift` floats past a 256-byte boundary, between 0xFF margins and canary guards."""

    def __init__(self, host, shift):
        import torch
        host = np.ascontiguousarray(host, np.float32)
        self.n, self.shift, nb = host.size, shift, host.size * 4
        self.g = _Guarded(nb + 32, GUARD, 0xFF)
        self.ptr = self.g.ptr + 4 * shift
        self.view = self.g.view[4 * shift:4 * shift + nb]
        self.view.copy_(torch.from_numpy(host.view(np.uint8)))

    def host(self):
        import torch
        torch.cuda.synchronize()
        assert self.g.guards_intact() == (True, True)
        raw = self.g.view.cpu().numpy()
        assert (raw[:4 * self.shift] == 0xFF).all() and (raw[4 * self.shift + 4 * self.n:] == 0xFF).all(), "margin written"
        return self.view.cpu().numpy().view(np.float32).copy()

    def f32(self):
        import torch
        return self.view.view(torch.float32)

    @property
    def p(self):
        return ctypes.c_void_p(self.ptr)


class _State(object):
    def __init__(self, lib, offs=OFFS, lens=LENS, decay=DECAY, fill=None):
        import torch
        self.lib, self.n_seg = lib, len(lens)
        self.lay = _i64([0] * 6)
        _lib.check(lib.ursn_opt_state_layout(_i64(lens), self.n_seg, self.lay))
        self.bytes = int(self.lay[0])
        assert self.bytes == lib.ursn_opt_state_size(_i64(lens), self.n_seg)
        self.g = _Guarded(self.bytes, GUARD, 0xFF)
        torch.cuda.synchronize()
        _lib.check(lib.ursn_opt_state_init(self.p, self.bytes, _i64(offs), _i64(lens), (ctypes.c_int32 * self.n_seg)(*decay), self.n_seg))
        if fill is not None:      # per-tensor results and chunk partials, after the init
            lo, hi = int(self.lay[2]), int(self.lay[3]) + 32 * int(self.lay[4])
            if fill == "nan64":
                self.g.view[lo:hi].view(torch.int64).fill_(NAN64)
            else:
                self.g.view[lo:hi].fill_(fill)
            torch.cuda.synchronize()

    @property
    def p(self):
        return ctypes.c_void_p(self.g.ptr)

    def read(self):
        st, rows = _lib.ursn_opt_status(), (_lib.ursn_opt_tensor * self.n_seg)()
        _lib.check(self.lib.ursn_opt_state_read(self.p, self.n_seg, ctypes.byref(st), rows, None))
        assert self.g.guards_intact() == (True, True)
        assert st.norm == math.sqrt(st.sumsq), "fp64 sqrt on the device is not correctly rounded: %r vs %r" % (st.norm, math.sqrt(st.sumsq))
        return st, rows


def _desc(lr=1e-3, clip=0.0, wd=0.0, skip=0):
    d = _lib.ursn_opt_desc()
    d.lr, d.clip_norm, d.weight_decay, d.skip_nonfinite = lr, clip, wd, skip
    return d


def _dyadic(seed, div, n=TOTAL):
    return (np.random.default_rng(seed).integers(-64, 65, n).astype(np.float64) / div).astype(np.float32)


def _random_state(seed, n=TOTAL):
    rng = np.random.default_rng(seed)
    p, g = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32)
    m, v = (rng.standard_normal(n) * 0.01).astype(np.float32), (rng.uniform(0, 1e-3, n)).astype(np.float32)
    return p, g, m, v


def _in_segments(n=TOTAL, infos=INFOS):
    mask = np.zeros(n, bool)
    for _, o, k, _ in infos:
        mask[o:o + k] = True
    return mask


def _guarded_step(lib, host4, shift, desc, t, state=None):
    """stats -> decide -> adam on fresh buffers; returns (p, m, v, status, rows, state)."""
    bufs = [_Buf(a, shift) for a in host4]
    state = state or _State(lib)
    _lib.check(lib.ursn_opt_stats(state.p, bufs[1].p, None, None))
    _lib.check(lib.ursn_opt_decide(state.p, ctypes.byref(desc), None))
    _lib.check(lib.ursn_opt_adam(state.p, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, TOTAL, ctypes.byref(desc), t, None))
    st, rows = state.read()
    assert same_bits(bufs[1].host(), host4[1]), "the gradient buffer was written"
    return bufs[0].host(), bufs[2].host(), bufs[3].host(), st, rows, state


def _plain_step(lib, host4, shift, lr, t, edit=None):
    """ursn_adam over the whole buffer from the same state; `edit(p_dev, g_dev)` may change the device tensors first (torch)."""
    bufs = [_Buf(a, shift) for a in host4]
    if edit is not None:
        edit(bufs[0].f32(), bufs[1].f32())
    _lib.check(lib.ursn_adam(bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, TOTAL, lr, 0.9, 0.999, 1e-8, t, None))
    return bufs[0].host(), bufs[2].host(), bufs[3].host()


def _assert_step_equal(got, want, before, what):
    """Inside the segments: the reference's bits; between them: untouched."""
    seg = _in_segments()
    for name, a, b, c in zip("pmv", got, want, before):
        assert same_bits(a[seg], b[seg]), "%s: %s differs in %d elements" % (what, name, int((a[seg].view(np.uint32) != b[seg].view(np.uint32)).sum()))
        assert same_bits(a[~seg], c[~seg]), "%s: %s written outside every segment" % (what, name)


def test_layout_constants(lib):
    lay = _i64([0] * 6)
    _lib.check(lib.ursn_opt_state_layout(_i64(LENS), len(LENS), lay))
    chunks = sum((n + CHUNK - 1) // CHUNK for n in LENS)
    assert lay[5] == CHUNK and lay[4] == chunks == 14 and lay[0] == 128 + 64 * len(LENS) + 48 * chunks


# ---- 1. sums bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_dyadic_sums_maxima_norm_and_coef_bit_for_bit(lib, shift):
    g, p = _dyadic(10 + shift, 32.0), _dyadic(20 + shift, 64.0)
    want = optim.grad_stats_numpy(g, p, INFOS)
    gb, pb, state = _Buf(g, shift), _Buf(p, (shift + 1) % 4), _State(lib)          # p placed differently inside its 16-byte line
    _lib.check(lib.ursn_opt_stats(state.p, gb.p, pb.p, None))
    st, rows = state.read()
    total = 0.0
    for i, (name, o, n, _) in enumerate(INFOS):
        assert rows[i].g_sumsq == np.sum(g[o:o + n].astype(np.float64) ** 2) == want[name]['grad_sumsq'], name
        assert rows[i].p_sumsq == np.sum(p[o:o + n].astype(np.float64) ** 2), name
        assert rows[i].g_maxabs == np.abs(g[o:o + n]).max() and rows[i].nonfinite == 0 and rows[i].reserved_ == 0, name
        total += rows[i].g_sumsq
    assert st.sumsq == total == want['global']['grad_sumsq'] and st.nonfinite == 0
    assert st.norm == np.sqrt(total) and (st.coef, st.skip, st.calls, st.skipped_total) == (1.0, 0, 0, 0)
    assert same_bits(gb.host(), g) and same_bits(pb.host(), p)
    # without parameters the parameter sums are written as 0
    _lib.check(lib.ursn_opt_stats(state.p, gb.p, None, None))
    st2, rows2 = state.read()
    assert all(r.p_sumsq == 0.0 for r in rows2) and [r.g_sumsq for r in rows2] == [r.g_sumsq for r in rows] and st2.sumsq == st.sumsq
    # the decision: one fp64 division rounded once; a clip above the norm leaves exactly 1
    clip = np.float32(st.norm / 3.0)
    d = _desc(clip=float(clip))
    _lib.check(lib.ursn_opt_decide(state.p, ctypes.byref(d), None))
    st3, _ = state.read()
    assert np.float32(st3.coef) == np.float32(float(clip) / st.norm) == optim.clip_coef_numpy(st.norm, clip) and st3.coef < 1
    assert (st3.skip, st3.calls, st3.skipped_total) == (0, 1, 0)
    d = _desc(clip=float(np.float32(st.norm * 1.5)))
    _lib.check(lib.ursn_opt_decide(state.p, ctypes.byref(d), None))
    st4, _ = state.read()
    assert np.float32(st4.coef).view(np.uint32) == 0x3F800000 and st4.calls == 2


def test_tensor_of_more_than_64_chunks(lib):
    """The one-workgroup pass adds a tensor's chunk partials 64 per round: 65 chunks and a ragged one reach its second round."""
    lens, gaps = [65 * CHUNK + 1, 7], [3, 2]
    offs, total = _table(lens, gaps)
    g = _dyadic(31, 32.0, total)
    g[offs[0] + 64 * CHUNK + 5] = np.inf
    state, gb = _State(lib, offs, lens, [1, 0]), _Buf(g, 1)
    _lib.check(lib.ursn_opt_stats(state.p, gb.p, None, None))
    st, rows = state.read()
    want = optim.grad_stats_numpy(g, None, [("a", offs[0], lens[0]), ("b", offs[1], lens[1])])
    assert (rows[0].g_sumsq, rows[0].nonfinite, rows[0].g_maxabs) == (want['a']['grad_sumsq'], 1, want['a']['grad_maxabs'])
    assert (rows[1].g_sumsq, rows[1].nonfinite) == (want['b']['grad_sumsq'], 0)
    assert st.sumsq == want['global']['grad_sumsq'] and st.nonfinite == 1 and math.isfinite(st.norm)


# ---- 2. scratch independence -----------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_state_held(lib):
    p, g, _, _ = _random_state(3)               # not dyadic: the bits now depend on the summation order
    runs = []
    for fill in (0x00, 0xFF, "nan64"):
        state, gb, pb = _State(lib, fill=fill), _Buf(g, 1), _Buf(p, 1)
        _lib.check(lib.ursn_opt_stats(state.p, gb.p, pb.p, None))
        st, rows = state.read()
        runs.append((bytes(st), bytes(rows)))
        if fill == 0x00:                       # and twice on one state
            _lib.check(lib.ursn_opt_stats(state.p, gb.p, pb.p, None))
            st, rows = state.read()
            runs.append((bytes(st), bytes(rows)))
    assert all(r == runs[0] for r in runs[1:])
    want = optim.grad_stats_numpy(g, p, INFOS)
    rows = (_lib.ursn_opt_tensor * len(LENS)).from_buffer_copy(runs[0][1])
    for i, (name, _, n, _) in enumerate(INFOS):  # fp64 round-off of the oracle: n * 2^-53 relative from the summation length
        assert abs(rows[i].g_sumsq - want[name]['grad_sumsq']) <= n * 2.0 ** -53 * want[name]['grad_sumsq'], name
        assert abs(rows[i].p_sumsq - want[name]['param_sumsq']) <= n * 2.0 ** -53 * want[name]['param_sumsq'], name
        assert rows[i].g_maxabs == want[name]['grad_maxabs']


# ---- 3. neutral equals plain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("shift", [0, 3])
def test_neutral_guarded_step_equals_ursn_adam(lib, t, shift):
    host4 = _random_state(40 + t)
    got = _guarded_step(lib, host4, shift, _desc(lr=1e-3), t)
    assert (got[3].coef, got[3].skip, got[3].nonfinite) == (1.0, 0, 0)
    want = _plain_step(lib, host4, shift, 1e-3, t)
    _assert_step_equal(got[:3], want, (host4[0], host4[2], host4[3]), "neutral t=%d" % t)
    assert not same_bits(got[0][_in_segments()], host4[0][_in_segments()])


# ---- 4. clipping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
def test_clipped_step_equals_ursn_adam_on_the_scaled_gradient(lib, shift):
    host4 = _random_state(50)
    norm = optim.grad_stats_numpy(host4[1], None, INFOS)['global']['grad_norm']
    clip = np.float32(norm / 3.0)
    got = _guarded_step(lib, host4, shift, _desc(lr=1e-3, clip=float(clip)), 5)
    coef = np.float32(got[3].coef)
    assert coef == np.float32(float(clip) / got[3].norm) and 0.3 < coef < 0.34        # from the device's own norm, as defined
    assert abs(got[3].norm - norm) <= TOTAL * 2.0 ** -53 * norm

    def scale(p_dev, g_dev):
        g_dev.mul_(float(coef))               # torch: one fp32 multiply per element

    want = _plain_step(lib, host4, shift, 1e-3, 5, edit=scale)
    _assert_step_equal(got[:3], want, (host4[0], host4[2], host4[3]), "clipped")
    plain = _plain_step(lib, host4, shift, 1e-3, 5)
    assert not same_bits(want[1], plain[1])
    # a clip above the norm: coef is exactly 1 and the step is the plain one
    got = _guarded_step(lib, host4, shift, _desc(lr=1e-3, clip=float(np.float32(norm * 2))), 5)
    assert np.float32(got[3].coef).view(np.uint32) == 0x3F800000
    _assert_step_equal(got[:3], plain, (host4[0], host4[2], host4[3]), "clip above the norm")


# ---- 5. decay --------------------------------------------------------------------------------------------------------------------
def test_decayed_step_equals_scaled_parameters_then_ursn_adam(lib):
    import torch
    host4 = _random_state(60)
    lr, wd = 2.0 ** -7, 0.125                 # exact in fp32: np.float32(1 - lr * wd) is the library's decay whichever way it is formed
    decay = np.float32(1 - lr * wd)
    assert decay == np.float32(1.0 - float(np.float32(lr)) * float(np.float32(wd))) and decay < 1
    got = _guarded_step(lib, host4, 2, _desc(lr=lr, wd=wd), 3)

    def shrink(p_dev, g_dev):
        for _, o, n, flag in INFOS:
            if flag:
                p_dev[o:o + n] *= float(decay)

    want = _plain_step(lib, host4, 2, lr, 3, edit=shrink)
    _assert_step_equal(got[:3], want, (host4[0], host4[2], host4[3]), "decay")
    plain = _plain_step(lib, host4, 2, lr, 3)
    for _, o, n, flag in INFOS:               # unflagged segments are the plain step, flagged ones are not
        assert same_bits(got[0][o:o + n], plain[0][o:o + n]) == (not flag)
    seg = _in_segments()
    assert same_bits(got[1][seg], plain[1][seg]) and same_bits(got[2][seg], plain[2][seg])        # the slots never see the decay


# ---- 6. skip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", SHIFTS)
def test_nonfinite_gradient_skips_the_step(lib, shift):
    """One NaN, +Inf, -Inf at: the single element of the length-1 segment; the last element of the longest segment, which lies in
    its ragged last chunk of 5 (the scalar tail or head of that chunk, depending on the shift); one in a full 16-byte vector."""
    host4 = _random_state(70)
    o_long, n_long = OFFS[LONGEST], LENS[LONGEST]
    where = [(0, OFFS[0]), (LONGEST, o_long + n_long - 1), (LONGEST, o_long + CHUNK + 37)]
    state, skips = _State(lib), 0
    clean = optim.grad_stats_numpy(host4[1], None, INFOS)
    for bad in (np.nan, np.inf, -np.inf):
        for seg, at in where:
            g = host4[1].copy()
            g[at] = bad
            p, m, v, st, rows, _ = _guarded_step(lib, (host4[0], g, host4[2], host4[3]), shift, _desc(clip=0.01, wd=0.1, skip=1), 2, state)
            skips += 1
            assert same_bits(p, host4[0]) and same_bits(m, host4[2]) and same_bits(v, host4[3]), (bad, at)
            assert (st.skip, st.nonfinite, st.calls, st.skipped_total) == (1, 1, skips, skips)
            assert [r.nonfinite for r in rows] == [int(i == seg) for i in range(len(LENS))]
            # the bad element contributes nothing: the sums are those of the buffer with a zero in its place
            want = optim.grad_stats_numpy(g, None, INFOS)
            assert math.isfinite(st.norm) and abs(st.sumsq - want['global']['grad_sumsq']) <= TOTAL * 2.0 ** -53 * st.sumsq
    # finite gradients on the same state: the step runs, the skip count stays
    p, m, v, st, rows, _ = _guarded_step(lib, host4, shift, _desc(skip=1), 2, state)
    assert (st.skip, st.nonfinite, st.calls, st.skipped_total) == (0, 0, skips + 1, skips)
    assert abs(st.sumsq - clean['global']['grad_sumsq']) <= TOTAL * 2.0 ** -53 * st.sumsq
    _assert_step_equal((p, m, v), _plain_step(lib, host4, shift, 1e-3, 2), (host4[0], host4[2], host4[3]), "after the skips")
    # skip_nonfinite = 0: the update runs (finite buffer only)
    p, m, v, st, _, _ = _guarded_step(lib, host4, shift, _desc(skip=0), 2)
    assert st.skip == 0 and not same_bits(p, host4[0])


# ---- 7. argument checks ----------------------------------------------------------------------------------------------------------
def test_refusals_on_device_memory(lib):
    import torch
    err = lambda: lib.ursn_last_error().decode()
    need = int(lib.ursn_opt_state_size(_i64(LENS), len(LENS)))
    mem = _Guarded(need + 64, GUARD, 0xFF)
    args = (_i64(OFFS), _i64(LENS), (ctypes.c_int32 * len(LENS))(*DECAY), len(LENS))
    assert lib.ursn_opt_state_init(ctypes.c_void_p(mem.ptr), need - 1, *args) != 0 and "too small" in err()
    assert lib.ursn_opt_state_init(ctypes.c_void_p(mem.ptr + 8), need, *args) != 0 and "16-byte aligned" in err()
    torch.cuda.synchronize()
    assert bool((mem.view == 0xFF).all().item()), "a refused init wrote the state"
    # a state nobody initialised: the launches touch nothing
    host4 = _random_state(80)
    bufs = [_Buf(a, 0) for a in host4]
    d = _desc()
    _lib.check(lib.ursn_opt_stats(ctypes.c_void_p(mem.ptr), bufs[1].p, None, None))
    _lib.check(lib.ursn_opt_decide(ctypes.c_void_p(mem.ptr), ctypes.byref(d), None))
    _lib.check(lib.ursn_opt_adam(ctypes.c_void_p(mem.ptr), bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, TOTAL, ctypes.byref(d), 1, None))
    torch.cuda.synchronize()
    assert bool((mem.view == 0xFF).all().item()) and mem.guards_intact() == (True, True)
    assert all(same_bits(b.host(), a) for a, b in zip(host4, bufs))
    st = _lib.ursn_opt_status()
    assert lib.ursn_opt_state_read(ctypes.c_void_p(mem.ptr), len(LENS), ctypes.byref(st), None, None) != 0 and "not built" in err()
    state = _State(lib)
    assert lib.ursn_opt_state_read(state.p, len(LENS) + 1, ctypes.byref(st), None, None) != 0 and "holds 8 tensors" in err()
    # buffers shorter than the table says: chunks that do not fit inside [0, n) are not touched
    _lib.check(lib.ursn_opt_stats(state.p, bufs[1].p, None, None))
    _lib.check(lib.ursn_opt_decide(state.p, ctypes.byref(d), None))
    cut = OFFS[5] + 10
    _lib.check(lib.ursn_opt_adam(state.p, bufs[0].p, bufs[1].p, bufs[2].p, bufs[3].p, cut, ctypes.byref(d), 1, None))
    p = bufs[0].host()
    assert same_bits(p[OFFS[5]:], host4[0][OFFS[5]:]) and not same_bits(p[OFFS[4]:OFFS[4] + LENS[4]], host4[0][OFFS[4]:OFFS[4] + LENS[4]])


def test_guarded_call_without_attached_state_is_refused():
    net = _build(NET_CASES[0])
    net.zero_gradients(None)
    lib, err = _lib.load(), lambda: _lib.load().ursn_last_error().decode()
    d, st = _desc(), _lib.ursn_opt_status()
    assert lib.ursn_apply_adam_guarded(net._handle, ctypes.byref(d), None) != 0 and "no optimiser state is attached (ursn_opt_attach)" in err()
    assert lib.ursn_grad_stats(net._handle, 1, None) != 0 and "no optimiser state is attached" in err()
    assert lib.ursn_opt_read(net._handle, ctypes.byref(st), None, None) != 0 and "no optimiser state is attached" in err()
    assert _adam_step(net) == 0
    net.set_optimizer(skip_nonfinite=True)
    _lib.check(lib.ursn_apply_adam_guarded(net._handle, ctypes.byref(d), None))
    _lib.check(lib.ursn_opt_attach(net._handle, None, 0))                        # NULL detaches
    assert lib.ursn_apply_adam_guarded(net._handle, ctypes.byref(d), None) != 0 and "no optimiser state is attached" in err()
    assert _adam_step(net) == 1


# ---- 8. net level ----------------------------------------------------------------------------------------------------------------
NET_CASES = [((16, 16, 16, 1), "fp32", 4, 2), ((16, 16, 16, 1), "bf16", 8, 2), ((32, 32, 1), "fp32", 4, 3)]
NET_IDS = ["%s_%s" % ("x".join(str(d) for d in c[0][:-1]), c[1]) for c in NET_CASES]
_inputs = {}


def _net_inputs(dims):
    if dims not in _inputs:
        ev = [sio.lartpc_sparse(dims, 3, e) for e in range(2)]
        _inputs[dims] = tuple(np.stack([e[j] for e in ev]) for j in range(3))
    return _inputs[dims]


def _build(case):
    dims, prec, base, ns = case
    net = uresnet(dims=list(dims), num_class=3, base_num_outputs=base, num_strides=ns)
    net.construct(trainable=True, use_weight=True, learning_rate=1e-3, seed=7, precision=prec)
    return net


def _iterate(net, case, lr=None):
    net.zero_gradients(None)
    net.accum_gradients(None, *_net_inputs(case[0]), fetch=False)
    net.apply_gradients(None) if lr is None else net.apply_gradients(None, lr=lr)


def _adam_step(net):
    t = ctypes.c_int64(-1)
    _lib.check(_lib.load().ursn_get_adam_step(net._handle, ctypes.byref(t)))
    return int(t.value)


def _same_vars(a, b):
    return sorted(a) == sorted(b) and all(same_bits(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", NET_CASES, ids=NET_IDS)
def test_net_grad_stats_equal_the_numpy_statement(case):
    net = _build(case)
    net.zero_gradients(None)
    net.accum_gradients(None, *_net_inputs(case[0]))
    got = net.grad_stats(None)
    g, p = net.get_gradients(), net.get_variables()
    want = optim.grad_stats_numpy(g, p)
    assert list(got) == net.variable_names() + ['global'] and sorted(got) == sorted(want)
    for name in net.variable_names():
        n, a, b = g[name].size, got[name], want[name]
        # counts and maxima exact; sums at fp64 round-off of the oracle, n * 2^-53 relative from the summation length
        assert a['nonfinite'] == b['nonfinite'] == 0 and a['grad_maxabs'] == b['grad_maxabs'], name
        assert abs(a['grad_sumsq'] - b['grad_sumsq']) <= n * 2.0 ** -53 * b['grad_sumsq'], (name, a['grad_sumsq'], b['grad_sumsq'])
        assert abs(a['param_sumsq'] - b['param_sumsq']) <= n * 2.0 ** -53 * b['param_sumsq'], (name, a['param_sumsq'], b['param_sumsq'])
        assert a['grad_norm'] == math.sqrt(a['grad_sumsq']) and a['param_norm'] == math.sqrt(a['param_sumsq'])
    n_all = sum(v.size for v in g.values())
    ga, gb = got['global'], want['global']
    assert ga['nonfinite'] == 0 and abs(ga['grad_sumsq'] - gb['grad_sumsq']) <= n_all * 2.0 ** -53 * gb['grad_sumsq']
    assert ga['grad_norm'] == math.sqrt(ga['grad_sumsq']) > 0
    assert any(v['param_norm'] == 0.0 for k, v in got.items() if k.endswith('/beta'))            # beta starts at 0
    quick = net.grad_stats(None, with_param_norms=False)
    assert all(quick[k]['param_sumsq'] == 0.0 and quick[k]['grad_sumsq'] == got[k]['grad_sumsq'] for k in net.variable_names())


@pytest.mark.parametrize("case", NET_CASES, ids=NET_IDS)
def test_net_neutral_optimizer_equals_the_plain_twin(case):
    twin, off, neutral = _build(case), _build(case), _build(case)
    off.set_optimizer()                                              # everything off: apply_gradients stays the plain call
    neutral.set_optimizer(clip_norm=1e30, skip_nonfinite=True)       # the guarded path with nothing to do
    start = twin.get_variables()
    for it in range(2):
        for net in (twin, off, neutral):
            _iterate(net, case)
        want = twin.get_variables()
        assert _same_vars(off.get_variables(), want), "set_optimizer() with everything off, iteration %d" % it
        assert _same_vars(neutral.get_variables(), want), "neutral guarded step, iteration %d" % it
    assert not _same_vars(want, start)
    assert same_bits(neutral._adam_m.cpu().numpy(), twin._adam_m.cpu().numpy())
    assert same_bits(neutral._adam_v.cpu().numpy(), twin._adam_v.cpu().numpy())
    st = neutral.last_apply_status(None)
    assert (st['calls'], st['skipped_total'], st['skip'], st['coef'], st['nonfinite'], st['lr']) == (2, 0, 0, 1.0, 0, 1e-3)
    assert st['norm'] == math.sqrt(st['sumsq']) > 0
    assert [_adam_step(n) for n in (twin, off, neutral)] == [2, 2, 2]
    assert off.last_apply_status(None)['calls'] == 0


@pytest.mark.parametrize("case", NET_CASES, ids=NET_IDS)
def test_net_poisoned_gradient_skips_one_step_and_training_goes_on(case):
    net = _build(case)
    net.set_optimizer(clip_norm=1.0, weight_decay=0.01, skip_nonfinite=True)
    before = net.get_variables()
    net.zero_gradients(None)
    net.accum_gradients(None, *_net_inputs(case[0]), fetch=False)
    net._grads[net._n_params // 2] = float("nan")                   # through the flat buffer view
    net.apply_gradients(None)
    assert _same_vars(net.get_variables(), before)
    assert not net._adam_m.any().item() and not net._adam_v.any().item()
    st = net.last_apply_status(None)
    assert (st['skip'], st['nonfinite'], st['calls'], st['skipped_total']) == (1, 1, 1, 1) and math.isfinite(st['norm'])
    stats = net.grad_stats(None, with_param_norms=False)
    assert sum(v['nonfinite'] for k, v in stats.items() if k != 'global') == 1 == stats['global']['nonfinite']
    _iterate(net, case)                                              # the next clean iteration trains
    after = net.get_variables()
    assert not _same_vars(after, before) and all(np.isfinite(v).all() for v in after.values())
    st = net.last_apply_status(None)
    assert (st['skip'], st['nonfinite'], st['calls'], st['skipped_total']) == (0, 0, 2, 1)
    assert _adam_step(net) == 2                                      # the counter advanced on the skipped step too
    # a larger batch re-creates the handle: the state is attached again and the cumulative counters carry over
    data, label, weight = _net_inputs(case[0])
    net.zero_gradients(None)
    net.accum_gradients(None, np.concatenate([data, data]), np.concatenate([label, label]), np.concatenate([weight, weight]), fetch=False)
    net.apply_gradients(None)
    st = net.last_apply_status(None)
    assert (st['skip'], st['calls'], st['skipped_total']) == (0, 3, 1) and _adam_step(net) == 3


# ---- 9. driver -------------------------------------------------------------------------------------------------------------------
def test_driver_keys(tmp_path, capsys):
    from uresnet_amd.ssnet_trainval import ssnet_trainval
    inp = tmp_path / "input.cfg"
    inp.write_text("Dims [32, 32, 1]\nNumClass 3\nGenerator 'lartpc_sparse'\nNumEntries 64\n"
                   "Keys {'data': 'main_data', 'label': 'main_label', 'weight': 'main_weight'}\n")
    cfg = tmp_path / "train.cfg"
    cfg.write_text("NUM_CLASS 3\nBASE_NUM_FILTERS 4\nMAIN_INPUT_CONFIG '%s'\nLOGDIR '%s'\nSAVE_FILE ''\nITERATIONS 3\nMINIBATCH_SIZE 2\n"
                   "NUM_MINIBATCHES 1\nLEARNING_RATE 0.001\nTRAIN True\nUSE_WEIGHTS True\nREPORT_STEPS 1\nSUMMARY_STEPS 1\n"
                   "CHECKPOINT_STEPS 0\nKEYWORD_DATA 'main_data'\nKEYWORD_LABEL 'main_label'\nKEYWORD_WEIGHT 'main_weight'\n"
                   "CLIP_GRAD_NORM 0.5\nSKIP_NONFINITE True\nGRAD_STATS True\nLR_WARMUP_STEPS 2\n" % (inp, tmp_path / "log"))
    t = ssnet_trainval()
    t.override_config(str(cfg))
    t.initialize()
    capsys.readouterr()
    lrs, calls = [], []
    for _ in range(3):
        t.train_step()
        st = t._net.last_apply_status(None)     # after grad_stats the decision fields are neutral again; lr and the counters stay
        lrs.append(st['lr'])
        calls.append(st['calls'])
    printed = capsys.readouterr().out
    want_lr = [optim.lr_at(t._cfg, it) for it in range(3)]
    assert want_lr == [0.0005, 0.001, 0.001] and lrs == want_lr and calls == [1, 2, 3]
    assert _adam_step(t._net) == 3
    names = t._net.variable_names()
    t.reset()
    assert re.findall(r"^@ iteration \d+ LR (\S+) Mem", printed, re.M) == ['0.0005', '0.001', '0.001']
    lines = re.findall(r"^Optimiser: gnorm=(\S+)   nonfinite=0   skipped=0$", printed, re.M)
    assert len(lines) == 3 and all(float(x) > 0 for x in lines)
    recs = [json.loads(x) for x in (tmp_path / "log" / "train" / "scalars.jsonl").read_text().strip().split("\n")]
    assert [r['iteration'] for r in recs] == [0, 1, 2] and [r['lr'] for r in recs] == want_lr
    for r in recs:
        assert np.isfinite(r['loss']) and r['gnorm'] > 0 and r['skipped_total'] == 0
        assert list(r['grad_norm']) == names and list(r['weight_norm']) == names
        assert all(np.isfinite(v) and v >= 0 for v in r['grad_norm'].values())
        assert all(r['weight_norm'][k] > 0 for k in names if k.endswith('/weights'))
        assert abs(math.sqrt(sum(v * v for v in r['grad_norm'].values())) - r['gnorm']) <= 1e-12 * r['gnorm']

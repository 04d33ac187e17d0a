"""Bare C-ABI driver for the state-independence tests: drives include/uresnet_hip.h through uresnet_amd._lib with buffers
the TEST owns.  The header says the four flat buffers and the workspace are caller-owned; ssnet.py hides the workspace behind
torch.empty (very often zero pages on a quiet process), so whether a call reads workspace bytes that nothing wrote can only be
seen from here: the workspace is filled with a chosen byte pattern BEFORE ursn_create (create's own clears must survive it),
every buffer sits between canary guards, and every comparison is on raw 32-bit patterns (NaN == NaN, +0 != -0).

Importable without a GPU (torch and the library are only touched when a Handle is built)."""
import ctypes

import numpy as np

from _net import as_f32_exact, oracle_params

FILLS = {"zero": 0x00,   # what a fresh allocation usually looks like
         "nan": 0xFF,    # 0xFFFFFFFF / 0xFFFF: a NaN as fp32 and as bf16
         "big": 0x7F}    # 0x7F7F7F7F / 0x7F7F: 3.39e38 as fp32 and as bf16, finite -- fmaxf(NaN, 0) == 0 hides a NaN in front of
#                          a ReLU, a huge finite value passes through it
CANARY = 0xA5
_SUFFIXES_FWD = (":z", ":mean", ":rstd", "")


def make_cfg(dims, base, ncls, num_strides, max_batch, trainable=1, use_weight=1, bf16=False, bn_eps=1e-3):
    from uresnet_amd import _lib
    cfg = _lib.ursn_config()
    cfg.ndim = len(dims) - 1
    for i in range(3):
        cfg.spatial[i] = int(dims[i]) if i < cfg.ndim else 1
    cfg.cin = int(dims[-1])
    cfg.base_filters, cfg.num_class, cfg.num_strides = int(base), int(ncls), int(num_strides)
    cfg.max_batch, cfg.trainable, cfg.use_weight = int(max_batch), int(trainable), int(use_weight)
    cfg.bn_eps = bn_eps
    cfg.act_dtype = 1 if bf16 else 0
    return cfg


def bits(a):
    """fp32 array -> its 32-bit patterns."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def upload(*arrays):
    """Host fp32 arrays -> device tensors, complete before this returns (None stays None)."""
    import torch
    out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


class _Guarded(object):
    """`nbytes` of device memory, 256-byte aligned, with at least `guard` canary bytes in front and `guard` behind."""

    def __init__(self, nbytes, guard, fill_byte):
        import torch
        self.nbytes = int(nbytes)
        self.raw = torch.full((guard + 256 + self.nbytes + guard,), CANARY, dtype=torch.uint8, device="cuda")
        base = self.raw.data_ptr()
        self.off = ((base + guard + 255) & ~255) - base
        self.ptr = base + self.off
        self.view = self.raw[self.off:self.off + self.nbytes]
        self.view.fill_(fill_byte)

    def guards_intact(self):
        front, back = self.raw[:self.off], self.raw[self.off + self.nbytes:]
        return bool((front == CANARY).all().item()), bool((back == CANARY).all().item())

    def f32(self):
        import torch
        return self.view.view(torch.float32)


class Handle(object):
    """One ursn_net over test-owned buffers.  `state` (optional): dict with host fp32 arrays params / grads / adam_m / adam_v and
    adam_step, the buffers as they stood before the call under test; default: oracle parameters (tests/_net.py, rounded with
    as_f32_exact, packed by ursn_param offsets like ssnet_base.set_variables), zero gradients and Adam slots, step 0."""

    def __init__(self, cfg, fill, guard=4096, state=None):
        import torch
        from uresnet_amd import _lib
        assert torch.cuda.is_available(), "tests/_abi.py: no HIP device visible"
        self._L, self.lib = _lib, _lib.load()
        self.cfg, self.fill, self.handle, self.last_n = cfg, fill, None, 0
        self.bf16 = cfg.act_dtype == 1
        self.sizes = _lib.ursn_sizes()
        _lib.check(self.lib.ursn_query(ctypes.byref(cfg), ctypes.byref(self.sizes)))
        npar = int(self.sizes.n_params)
        self.spatial = tuple(int(cfg.spatial[i]) for i in range(cfg.ndim))
        self.pix = int(np.prod(self.spatial))
        self.params = _Guarded(npar * 4, guard, 0)
        self.grads = self.adam_m = self.adam_v = None
        if cfg.trainable:
            self.grads, self.adam_m, self.adam_v = (_Guarded(npar * 4, guard, 0) for _ in range(3))
        self.ws = _Guarded(int(self.sizes.workspace_bytes), guard, FILLS[fill])   # filled BEFORE create
        torch.cuda.synchronize()
        h = ctypes.c_void_p()
        p = lambda g: ctypes.c_void_p(g.ptr) if g is not None else None
        _lib.check(self.lib.ursn_create(ctypes.byref(cfg), p(self.params), p(self.grads), p(self.adam_m), p(self.adam_v),
                                        ctypes.c_void_p(self.ws.ptr), self.ws.nbytes, ctypes.byref(h)))
        self.handle = h
        if state is None:
            state = {"params": self._oracle_params()}
        self.params.f32().copy_(torch.from_numpy(np.ascontiguousarray(state["params"], dtype=np.float32)))
        if cfg.trainable:
            for name in ("grads", "adam_m", "adam_v"):
                if state.get(name) is not None:
                    getattr(self, name).f32().copy_(torch.from_numpy(np.ascontiguousarray(state[name], dtype=np.float32)))
        _lib.check(self.lib.ursn_set_adam_step(self.handle, int(state.get("adam_step", 0))))
        torch.cuda.synchronize()

    # ---- parameters ---------------------------------------------------------------------------------------------------
    def _oracle_params(self):
        cfg = self.cfg
        dims = self.spatial + (int(cfg.cin),)
        P = as_f32_exact(oracle_params(dims, int(cfg.base_filters), int(cfg.num_class), num_strides=int(cfg.num_strides)))
        host = np.zeros(int(self.sizes.n_params), np.float32)
        info = self._L.ursn_param_info()
        seen = 0
        for i in range(int(self.sizes.n_tensors)):
            self._L.check(self.lib.ursn_param(self.handle, i, ctypes.byref(info)))
            v = np.asarray(P[info.name.decode()], np.float32).reshape(-1)
            assert v.size == info.nelem, (info.name, v.size, info.nelem)
            host[info.offset:info.offset + info.nelem] = v
            seen += int(info.nelem)
        assert seen == host.size, (seen, host.size)
        return host

    # ---- lifecycle ----------------------------------------------------------------------------------------------------
    def destroy(self):
        if self.handle is not None:
            import torch
            torch.cuda.synchronize()
            self._L.check(self.lib.ursn_destroy(self.handle))
            self.handle = None

    def check_guards(self):
        """An out-of-bounds WRITE next to any of the five buffers shows here."""
        import torch
        torch.cuda.synchronize()
        for name in ("params", "grads", "adam_m", "adam_v", "ws"):
            g = getattr(self, name)
            if g is not None:
                front, back = g.guards_intact()
                assert front and back, "canary guard of %s overwritten (front intact: %s, back intact: %s)" % (name, front, back)

    def close(self):
        self.destroy()
        self.check_guards()

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            self.close()
        else:   # keep the first failure; still release the handle
            try:
                self.destroy()
            except Exception:
                pass
        return False

    # ---- host copies --------------------------------------------------------------------------------------------------
    @staticmethod
    def _host(t):
        import torch
        torch.cuda.synchronize()
        return t.cpu().numpy().copy()

    def host(self, name):
        g = getattr(self, name)
        return None if g is None else self._host(g.f32())

    def adam_step(self):
        t = ctypes.c_int64(0)
        self._L.check(self.lib.ursn_get_adam_step(self.handle, ctypes.byref(t)))
        return int(t.value)

    def state(self):
        return {"params": self.host("params"), "grads": self.host("grads"), "adam_m": self.host("adam_m"),
                "adam_v": self.host("adam_v"), "adam_step": self.adam_step()}

    # ---- the fetch-sets -----------------------------------------------------------------------------------------------
    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    @staticmethod
    def _s(stream):
        if stream is None:
            return None
        return ctypes.c_void_p(getattr(stream, "cuda_stream", stream))

    def zero_grad(self, stream=None, fetch=True):
        self._L.check(self.lib.ursn_zero_grad(self.handle, self._s(stream)))
        return {"grads": self.host("grads")} if fetch else None

    def accum_step(self, data, label, weight, n, stream=None, fetch=True):
        """fetch=False: out3 = NULL, the call only enqueues and nothing is read back."""
        out = (ctypes.c_float * 3)(*([float("nan")] * 3))
        self.last_n = n
        self._L.check(self.lib.ursn_accum_step(self.handle, self._p(data), self._p(label), self._p(weight), n,
                                               out if fetch else None, self._s(stream)))
        if not fetch:
            return None
        return {"metrics": np.array(list(out), np.float32), "grads": self.host("grads")}

    def apply_adam(self, lr=1e-3, stream=None, fetch=True):
        self._L.check(self.lib.ursn_apply_adam(self.handle, lr, self._s(stream)))
        if not fetch:
            return None
        return {"params": self.host("params"), "adam_m": self.host("adam_m"), "adam_v": self.host("adam_v")}

    def eval(self, data, label, weight, n, stream=None):
        out = (ctypes.c_float * 3)(*([float("nan")] * 3))
        self.last_n = n
        self._L.check(self.lib.ursn_eval(self.handle, self._p(data), self._p(label), self._p(weight), n, out, self._s(stream)))
        return {"metrics": np.array(list(out), np.float32)}

    def _nan_out(self, *shape):
        import torch
        t = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")   # an element the call leaves unwritten stays NaN
        torch.cuda.synchronize()
        return t

    def infer(self, data, label, n, stream=None):
        sm = self._nan_out(n, self.pix, int(self.cfg.num_class))
        out = (ctypes.c_float * 2)(*([float("nan")] * 2))
        self.last_n = n
        self._L.check(self.lib.ursn_infer(self.handle, self._p(data), self._p(label), n, self._p(sm), out, self._s(stream)))
        res = {"softmax_out": self._host(sm)}
        if label is not None:
            res["metrics"] = np.array(list(out), np.float32)
        return res

    def infer_labels(self, data, label, n, stream=None, with_softmax=True):
        lab = self._nan_out(n, self.pix)
        sm = self._nan_out(n, self.pix, int(self.cfg.num_class)) if with_softmax else None
        out = (ctypes.c_float * 2)(*([float("nan")] * 2))
        self.last_n = n
        self._L.check(self.lib.ursn_infer_labels(self.handle, self._p(data), self._p(label), n, self._p(lab), self._p(sm), out,
                                                 self._s(stream)))
        res = {"labels_out": self._host(lab)}
        if with_softmax:
            res["softmax_out"] = self._host(sm)
        if label is not None:
            res["metrics"] = np.array(list(out), np.float32)
        return res

    def read_metrics(self, stream=None):
        out = (ctypes.c_float * 3)(*([float("nan")] * 3))
        self._L.check(self.lib.ursn_read_metrics(self.handle, out, self._s(stream)))
        return {"metrics": np.array(list(out), np.float32)}

    # ---- stored tensors (diagnostics) ---------------------------------------------------------------------------------
    def layer_names(self):
        info = self._L.ursn_layer_info()
        names = []
        for i in range(int(self.sizes.n_layers)):
            self._L.check(self.lib.ursn_query_layer(ctypes.byref(self.cfg), i, ctypes.byref(info)))
            names.append(info.name.decode())
        return names

    def tensor(self, name):
        """Raw elements of a stored tensor of the last call as [n * voxels, cstride] (uint32 patterns on the fp32 plan, uint16
        on the bf16 plan; the pad lanes of the last voxel of a channel-slice view, which lie outside it, read as 0), or
        [channels] uint32 for :mean / :rstd, plus the channel count.  None: the plan does not hold this tensor."""
        ptr, vox, ch, cs = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        if self.lib.ursn_tensor(self.handle, name.encode(), ctypes.byref(ptr), ctypes.byref(vox), ctypes.byref(ch),
                                ctypes.byref(cs)) != 0 or not ptr.value:
            return None   # "not materialised", "no second gradient tensor", "no activation named", not trainable
        off = ptr.value - self.ws.ptr
        if vox.value == 0:
            nbytes, dt = ch.value * 4, np.uint32
        else:
            esz = 2 if self.bf16 else 4
            total = int(self.last_n * vox.value * cs.value)
            nbytes, dt = (total - (cs.value - ch.value)) * esz, (np.uint16 if self.bf16 else np.uint32)
        assert 0 <= off and off + nbytes <= self.ws.nbytes, "%s lies outside the workspace" % name
        raw = self._host(self.ws.view[off:off + nbytes]).view(dt)
        if vox.value == 0:
            return raw, ch.value
        full = np.zeros(total, dt)
        full[:raw.size] = raw
        return full.reshape(-1, cs.value), ch.value


def tensor_order(layer_names):
    """ursn_tensor names in execution order.  A residual unit's join is stored under the unit's scope (the parent of its
    resnet_conv2), every other activation under its layer's scope; the bf16 plan's second level-0 gradient tensor is
    UResNet/conv0:grad2."""
    fwd, bwd = [], []
    for n in layer_names:
        fwd += [n + s for s in _SUFFIXES_FWD]
        if n.endswith("/resnet_conv2"):
            fwd.append(n[:-len("/resnet_conv2")])
    for n in reversed(layer_names):
        if n.endswith("/resnet_conv2"):
            bwd.append(n[:-len("/resnet_conv2")] + ":grad")
        bwd += [n + ":grad", n + ":dz"]
        if n == "UResNet/conv0":
            bwd.insert(len(bwd) - 1, n + ":grad2")
    return fwd + ["logits:grad"] + bwd


def first_difference(ha, hb):
    """First stored tensor, in execution order (forward: :z, :mean, :rstd, activation of every layer; then backward:
    logits:grad, and :dz, :grad of every layer in reverse), whose bits differ between the two handles' last calls, over the
    WHOLE channel stride, and whether the difference sits in the `channels` lanes or only in the pad.  Diagnostic for assertion
    messages only: pad lanes that nobody writes and nobody reads may keep the fill, so a difference reported here is a lead,
    not a verdict."""
    if ha.handle is None or hb.handle is None:
        return "first difference: a handle is already destroyed"
    order = tensor_order(ha.layer_names())
    compared = 0
    for name in order:
        ta, tb = ha.tensor(name), hb.tensor(name)
        if ta is None or tb is None:
            continue
        (a, ch), (b, _) = ta, tb
        if a.shape != b.shape:
            return "first difference: %s has shape %s against %s" % (name, a.shape, b.shape)
        compared += 1
        ne = a != b
        if not ne.any():
            continue
        if a.ndim == 1:
            return "first difference: %s, %d of %d elements (fills %s / %s)" % (name, int(ne.sum()), ne.size, ha.fill, hb.fill)
        inch, inpad = int(ne[:, :ch].sum()), int(ne[:, ch:].sum())
        where = "in the channel lanes" if inpad == 0 else "ONLY in the pad lanes" if inch == 0 else "in channel and pad lanes"
        return ("first difference: %s, %d of %d elements differ %s (%d in the %d channel lanes, %d in the %d pad lanes; first "
                "voxel %d; fills %s / %s)" % (name, inch + inpad, ne.size, where, inch, ch, inpad, a.shape[1] - ch,
                                              int(np.argmax(ne.any(axis=1))), ha.fill, hb.fill))
    return "first difference: none among the %d stored tensors compared (fills %s / %s)" % (compared, ha.fill, hb.fill)


def compare_outputs(what, out_a, out_b, ha, hb):
    """Bitwise equality of two calls' outputs (dicts of fp32 arrays); the message names the output, how many elements differ
    and first_difference's layer."""
    assert (out_a is None) == (out_b is None), what
    if out_a is None:
        return
    assert sorted(out_a) == sorted(out_b), (what, sorted(out_a), sorted(out_b))
    for k in sorted(out_a):
        a, b = out_a[k], out_b[k]
        if a is None and b is None:
            continue
        if not same_bits(a, b):
            nd = int((bits(a) != bits(b)).sum()) if a.shape == b.shape else -1
            raise AssertionError("%s: %s differs in %d of %d elements (%s); %s"
                                 % (what, k, nd, a.size, _sample(a, b), first_difference(ha, hb)))


def _sample(a, b):
    if a.shape != b.shape:
        return "shapes %s / %s" % (a.shape, b.shape)
    i = int(np.argmax((bits(a) != bits(b)).reshape(-1)))
    return "first at %d: %r / %r" % (i, float(a.reshape(-1)[i]), float(b.reshape(-1)[i]))

"""Python 3 mirror of the reference plugin surface lib/ssnet.py (class ssnet_base).

Same constructor, same abstract ``_build`` hook, same ``construct`` signature and the same six
run methods with the same return structures (lib/ssnet.py:91-153).  Where the reference builds a
TensorFlow graph and each method is one ``sess.run`` fetch-set, here ``construct`` records the
topology symbolically, checks it against the launch plan compiled into liburesnet_hip.so and
each method is one call through the C-ABI (include/uresnet_hip.h).  PyTorch-ROCm only provides
device memory, streams and the RCCL process group.  There is no CPU fallback.
"""
from __future__ import print_function

import ctypes
import math
import sys

import numpy as np

from . import _lib
from .resnet_module import Graph, SymTensor


class _NoMovingStatistics(RuntimeError, ValueError):
    """``set_bn_mode('frozen')`` on a network without moving statistics: a missing buffer (the RuntimeError every other entry
    raises for it) and a mode this network cannot take (the ValueError an unknown mode raises)."""


class HipSession(object):
    """Stands in for ``tf.Session`` (lib/ssnet_trainval.py:112): names the device and stream the
    fetch-sets run on.  Every run method also accepts ``sess=None`` (current device/stream)."""

    def __init__(self, device=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('HipSession: no HIP device visible; the U-ResNet path has no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else int(device))

    def stream_ptr(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class _Adam(object):
    """Carries ``_lr`` like tf.train.AdamOptimizer (read at lib/ssnet_trainval.py:209)."""

    def __init__(self, lr):
        self._lr = lr
        self._beta1, self._beta2, self._epsilon = 0.9, 0.999, 1e-8


class VoxelBatch(object):
    """A minibatch as larcv-style voxel lists (not in the reference's Python surface, which only sees the dense arrays larcv
    fills; its ana OUTPUT is this form: lib/ssnet_trainval.py:299-302).  Event i owns list entries
    ``[offsets[i], offsets[i+1])``; ``index`` is the row-major voxel index inside the event, strictly increasing per event;
    every voxel not listed is ``(data, label, weight) = (0, 0, bg_weight[i])``.  ``label`` / ``weight`` (with ``bg_weight``) may
    be None.  Mirrors ``ursn_voxel_batch`` (include/uresnet_hip.h)."""

    __slots__ = ('offsets', 'index', 'value', 'label', 'weight', 'bg_weight', 'voxels')

    def __init__(self, offsets, index, value, label=None, weight=None, bg_weight=None, voxels=0):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.index = np.ascontiguousarray(index, dtype=np.int32)
        self.value = np.ascontiguousarray(value, dtype=np.float32)
        self.label = None if label is None else np.ascontiguousarray(label, dtype=np.float32)
        self.weight = None if weight is None else np.ascontiguousarray(weight, dtype=np.float32)
        self.bg_weight = None if bg_weight is None else np.ascontiguousarray(bg_weight, dtype=np.float32)
        self.voxels = int(voxels)

    @property
    def n(self):
        return int(self.offsets.shape[0]) - 1

    def validate(self):
        """O(M) host check of everything the device passes take on trust; raises ValueError naming the first offence."""
        off, idx, V = self.offsets, self.index, self.voxels
        if not 1 <= V < 2 ** 31:
            raise ValueError('VoxelBatch: voxels = %d outside [1, 2^31)' % V)
        if off.ndim != 1 or off.shape[0] < 2:
            raise ValueError('VoxelBatch: offsets must be a 1-D array of n + 1 >= 2 entries')
        if off[0] != 0:
            raise ValueError('VoxelBatch: offsets[0] = %d, must be 0' % off[0])
        bad = np.flatnonzero(np.diff(off) < 0)
        if bad.size:
            raise ValueError('VoxelBatch: offsets decrease at event %d (%d -> %d)' % (bad[0], off[bad[0]], off[bad[0] + 1]))
        M = int(off[-1])
        for name in ('index', 'value', 'label', 'weight'):
            a = getattr(self, name)
            if a is not None and (a.ndim != 1 or a.shape[0] != M):
                raise ValueError('VoxelBatch: %s has shape %s, offsets[-1] says %d entries' % (name, a.shape, M))
        if (self.weight is None) != (self.bg_weight is None):
            raise ValueError('VoxelBatch: weight and bg_weight must be given together')
        if self.bg_weight is not None and self.bg_weight.shape != (self.n,):
            raise ValueError('VoxelBatch: bg_weight has shape %s for %d events' % (self.bg_weight.shape, self.n))
        bad = np.flatnonzero((idx < 0) | (idx >= V))
        if bad.size:
            j = int(bad[0])
            raise ValueError('VoxelBatch: index[%d] = %d outside [0, %d) (event %d)'
                             % (j, idx[j], V, int(np.searchsorted(off, j, side='right')) - 1))
        if M > 1:
            step = np.diff(idx) <= 0
            seams = off[1:-1] - 1            # entry pairs that straddle two events carry no order
            step[seams[(seams >= 0) & (seams < M - 1)]] = False
            bad = np.flatnonzero(step)
            if bad.size:
                j = int(bad[0])
                raise ValueError('VoxelBatch: indices must be strictly increasing inside an event: index[%d] = %d is followed '
                                 'by %d (event %d)' % (j, idx[j], idx[j + 1], int(np.searchsorted(off, j, side='right')) - 1))
        return self

    def normalize_weights(self):
        """The per-event normalisation of lib/ssnet_trainval.py:173 (weight /= sum over the event) on the list: ``weight`` and
        ``bg_weight`` divided, in place, by sum(listed w) + (voxels - m_i) * bg_weight[i] formed in float64."""
        for i in range(self.n):
            a, b = int(self.offsets[i]), int(self.offsets[i + 1])
            total = float(np.sum(self.weight[a:b], dtype=np.float64)) + float(self.voxels - (b - a)) * float(self.bg_weight[i])
            self.weight[a:b] = (self.weight[a:b].astype(np.float64) / total).astype(np.float32)
            self.bg_weight[i] = np.float32(float(self.bg_weight[i]) / total)
        return self

    @staticmethod
    def concat(batches):
        """Events of several batches (same ``voxels``, same optional roles) as one batch."""
        batches = list(batches)
        V = batches[0].voxels
        if any(b.voxels != V for b in batches):
            raise ValueError('VoxelBatch.concat: events of different sizes')
        counts = np.concatenate([np.diff(b.offsets) for b in batches])
        off = np.zeros(counts.shape[0] + 1, np.int64)
        np.cumsum(counts, out=off[1:])

        def cat(name):
            parts = [getattr(b, name) for b in batches]
            if any(p is None for p in parts):
                if not all(p is None for p in parts):
                    raise ValueError('VoxelBatch.concat: %s present in some batches only' % name)
                return None
            return np.concatenate(parts)
        return VoxelBatch(off, cat('index'), cat('value'), cat('label'), cat('weight'), cat('bg_weight'), V)


class _DeviceVoxelBatch(object):
    """What ``ssnet_base.upload_voxels`` returns: a large VoxelBatch resident on the device.  ``dev`` owns the memory, ``ptr`` maps
    the array names to device addresses, ``big`` is the events' shape, ``n`` / ``m`` the events and list entries; ``offsets`` /
    ``index`` are host copies (results are split and labelled with them), ``weight`` is None iff there is no weight list."""

    __slots__ = ('dev', 'ptr', 'big', 'n', 'm', 'offsets', 'index', 'weight')


def class_stats_from_counts(conf, other, score_sum, score_sq, nonzero=None):
    """The per-event quantities of example_scripts/ana_csv.py:67-116 from what ``ursn_class_stats`` returns: ``conf`` [n, C, C]
    (label, prediction) counts, ``other`` [n, 2] labels outside [0, C) {> 0, the rest}, ``score_sum`` / ``score_sq`` [n, C] fp64 sums
    of each class's score over the voxels that carry it, ``nonzero`` [n, 2] {data > 0, of those correct} or None.  Returns a dict
    of numpy arrays; the reference's sentinels: -1.0 in ``acc_class`` / ``score_mean`` / ``score_std`` where ``npx == 0``
    (ana_csv.py:99-101), NaN where an accuracy has no voxel to be taken over.  A label that is not an integer counts as the class
    it truncates to (the network's cast), where the reference's ``prediction == label`` never holds for it."""
    conf = np.asarray(conf, dtype=np.int64)
    other = np.asarray(other, dtype=np.int64)
    ssum, ssq = np.asarray(score_sum, dtype=np.float64), np.asarray(score_sq, dtype=np.float64)
    n = conf.shape[0]
    npx = conf.sum(axis=2)
    diag = np.diagonal(conf, axis1=1, axis2=2)
    some = npx > 0
    den = np.where(some, npx, 1).astype(np.float64)
    mean = ssum / den
    std = np.sqrt(np.maximum(ssq / den - mean * mean, 0.0))     # population std: numpy's .std()
    voxels = conf.sum(axis=(1, 2)) + other.sum(axis=1)

    def ratio(num, cnt):
        return np.where(cnt > 0, num / np.where(cnt > 0, cnt, 1).astype(np.float64), np.nan)
    res = {'conf': conf, 'other': other, 'npx': npx,
           'acc_class': np.where(some, diag / den, -1.0),
           'score_mean': np.where(some, mean, -1.0),
           'score_std': np.where(some, std, -1.0),
           'acc_all': diag.sum(axis=1) / voxels.astype(np.float64),
           # ana_csv.py:81-84: over label > 0, i.e. classes >= 1 plus the labels >= C (which match no prediction)
           'acc_nonzero_label': ratio(diag[:, 1:].sum(axis=1), npx[:, 1:].sum(axis=1) + other[:, 0])}
    if nonzero is None:
        res['acc_nonzero_data'] = np.full(n, np.nan)
    else:
        nz = np.asarray(nonzero, dtype=np.int64)
        res['acc_nonzero_data'] = ratio(nz[:, 1], nz[:, 0])
    return res


def ana_csv_header(num_class):
    """The header line of example_scripts/ana_csv.py:30-37."""
    return 'entry,acc_all,acc_nonzero' + ''.join(
        ',npx_class%d,acc_class%d,mean_softmax_class%d,std_softmax_class%d' % (i, i, i, i) for i in range(num_class)) + '\n'


def ana_csv_row(entry, stats, i):
    """Event ``i`` of an ``inference_stats`` result as the reference's CSV row (example_scripts/ana_csv.py:87,113-116)."""
    row = '%d,%g,%g' % (entry, stats['acc_all'][i], stats['acc_nonzero_label'][i])
    for k in range(stats['npx'].shape[1]):
        row += ',%d,%g,%g,%g' % (stats['npx'][i, k], stats['acc_class'][i, k], stats['score_mean'][i, k], stats['score_std'][i, k])
    return row + '\n'


def objects_csv_header():
    """The header line of the ANA_OBJECTS file: one row per cluster."""
    cols = ['entry', 'cluster', 'class', 'size', 'charge']
    for name in ('centroid', 'eval', 'axis'):
        cols += ['%s_%d' % (name, a) for a in range(3)]
    cols.append('length')
    for name in ('end_lo', 'end_hi'):
        cols += ['%s_%d' % (name, a) for a in range(3)]
    return ','.join(cols) + '\n'


def profiles_csv_header():
    """The header line of the ANA_PROFILES file: one row per cluster."""
    from .clusters import PROFILE_ROW_INT, PROFILE_ROW_REAL
    return ','.join(('entry', 'cluster') + PROFILE_ROW_INT + PROFILE_ROW_REAL) + '\n'


def profiles_csv_row(entry, k, rows):
    """Cluster ``k`` of one event's profile ``rows`` record (a dict of columns) as a CSV row: the twelve integers, then the six
    reals by ``repr`` (which reads back to the same bits)."""
    from .clusters import PROFILE_ROW_INT, PROFILE_ROW_REAL
    return ','.join(['%d' % entry, '%d' % k] + ['%d' % int(rows[name][k]) for name in PROFILE_ROW_INT] +
                    [repr(float(rows[name][k])) for name in PROFILE_ROW_REAL]) + '\n'


def split_csv_header():
    """The header line of the ANA_SPLIT file: one row per junction."""
    from .clusters import SPLIT_JUNCTION_INT, SPLIT_JUNCTION_REAL
    return ','.join(('entry', 'junction') + SPLIT_JUNCTION_INT + SPLIT_JUNCTION_REAL) + '\n'


def split_csv_row(entry, k, junctions):
    """Junction ``k`` of one event's ``junctions`` record (a dict of columns) as a CSV row: the integers, then the reals by
    ``repr`` (which round-trips a float64)."""
    from .clusters import SPLIT_JUNCTION_INT, SPLIT_JUNCTION_REAL
    return ','.join(['%d' % entry, '%d' % k] + ['%d' % int(junctions[name][k]) for name in SPLIT_JUNCTION_INT] +
                    [repr(float(junctions[name][k])) for name in SPLIT_JUNCTION_REAL]) + '\n'


def chains_csv_header():
    """The header line of the ANA_CHAINS file: one row per chain."""
    from .clusters import CHAIN_INT, CHAIN_REAL
    return ','.join(('entry', 'chain') + CHAIN_INT + CHAIN_REAL) + '\n'


def chains_csv_row(entry, k, chains):
    """Chain ``k`` of one event's ``chains`` record (a dict of columns) as a CSV row: the integers, then the reals by ``repr``
    (they parse back to the same bits)."""
    from .clusters import CHAIN_INT, CHAIN_REAL
    return ','.join(['%d' % entry, '%d' % k] + ['%d' % int(chains[name][k]) for name in CHAIN_INT] +
                    [repr(float(chains[name][k])) for name in CHAIN_REAL]) + '\n'


def cones_csv_header():
    """The header line of the ANA_CONES file: one row per shower."""
    from .clusters import CONE_INT, CONE_REAL
    return ','.join(('entry', 'shower') + CONE_INT + CONE_REAL) + '\n'


def cones_csv_row(entry, k, showers):
    """Shower ``k`` of one event's ``showers`` record (a dict of columns) as a CSV row: the integers, then the reals by ``repr``
    (which parses back to the same double)."""
    from .clusters import CONE_INT, CONE_REAL
    return ','.join(['%d' % entry, '%d' % k] + ['%d' % int(showers[name][k]) for name in CONE_INT] +
                    [repr(float(showers[name][k])) for name in CONE_REAL]) + '\n'


def vertices_csv_header():
    """The header line of the ANA_VERTICES file: one row per vertex."""
    from .clusters import VERTEX_INT, VERTEX_REAL
    return ','.join(('entry', 'vertex') + VERTEX_INT + VERTEX_REAL) + '\n'


def vertices_csv_row(entry, k, vertices):
    """Vertex ``k`` of one event's ``vertices`` record (a dict of columns) as a CSV row: the integers, then the reals by ``repr``
    (which reads back to the same bits)."""
    from .clusters import VERTEX_INT, VERTEX_REAL
    return ','.join(['%d' % entry, '%d' % k] + ['%d' % int(vertices[name][k]) for name in VERTEX_INT] +
                    [repr(float(vertices[name][k])) for name in VERTEX_REAL]) + '\n'


def match_csv_header():
    """The header line of the ANA_MATCH file: one row per event."""
    from .clusters import MATCH_EVENT_INT, MATCH_EVENT_REAL
    return ','.join(('entry',) + MATCH_EVENT_INT + MATCH_EVENT_REAL) + '\n'


def match_csv_row(entry, events, i):
    """Event ``i`` of a match's ``events`` record as a CSV row: the twelve integers, then the four reals by ``repr`` (which reads
    back to the same bits)."""
    from .clusters import MATCH_EVENT_INT, MATCH_EVENT_REAL
    return ','.join(['%d' % entry] + ['%d' % int(events[name][i]) for name in MATCH_EVENT_INT] +
                    [repr(float(events[name][i])) for name in MATCH_EVENT_REAL]) + '\n'


def graph_csv_header():
    """The header line of the ANA_GRAPH file: one row per interaction group."""
    from .clusters import GRAPH_GROUP
    return ','.join(('entry', 'group') + GRAPH_GROUP) + '\n'


def graph_csv_row(entry, g, groups):
    """Group ``g`` of one event's ``groups`` record (a dict of columns, ``clusters.GRAPH_GROUP``) as a CSV row of integers."""
    from .clusters import GRAPH_GROUP
    return ','.join(['%d' % entry, '%d' % g] + ['%d' % int(groups[name][g]) for name in GRAPH_GROUP]) + '\n'


def objects_csv_row(entry, k, objects, index, start, shape):
    """Cluster ``k`` of one event's ``objects`` record as a CSV row.  ``index`` is the event's index list, ``start`` the list position
    of its first entry (``end_lo`` / ``end_hi`` count from the start of the batch), ``shape`` the shape the indices are row-major in.
    The charge is the fixed-point sum divided by 2^16; floats are written with 17 significant digits and read back to the same bits."""
    o = objects
    row = '%d,%d,%d,%d,%.17g' % (entry, k, o['cls'][k], o['size'][k], float(int(o['charge'][k])) / 65536.0)
    for name in ('centroid', 'eval', 'axis'):
        row += ''.join(',%.17g' % x for x in o[name][k])
    row += ',%.17g' % o['length'][k]
    for name in ('end_lo', 'end_hi'):
        c = np.unravel_index(int(index[int(o[name][k]) - int(start)]), tuple(int(s) for s in shape))
        row += ''.join(',%d' % (int(c[a]) if a < len(c) else 0) for a in range(3))
    return row + '\n'


class ssnet_base(object):

    def __init__(self, dims, num_class):
        self._dims = np.array(dims, np.int32)
        if not len(self._dims) in [3, 4]:
            print('Error: len(dims) =', len(self._dims), 'but only 3 (H,W,C) or 4 (H,W,D,C) supported!')
            raise NotImplementedError
        self._num_class = int(num_class)
        self._handle = None
        self._max_batch = 0
        self._params = None

    def _build(self, input_tensor):
        raise NotImplementedError

    # ------------------------------------------------------------------------------------------
    # construct (lib/ssnet.py:20-89)
    # ------------------------------------------------------------------------------------------
    def construct(self, trainable=True, use_weight=True, learning_rate=None, allocate=True, device=None,
                  seed=1234, bn_eps=1e-3, precision='fp32', bn_moving=False, bn_decay=0.999):
        """``precision='bf16'`` (not in the reference, which is fp32 TensorFlow): mixed precision -- activations and
        gradient tensors bf16 in HBM, bf16 MFMA convolutions with fp32 accumulation; parameters, BatchNorm statistics,
        accumulated gradients and Adam stay fp32 (BASELINE.json configs[4]).

        ``bn_moving`` (the half of slim.batch_norm the reference leaves dead): allocates the moving statistics of every
        BatchNorm layer (mean 0, variance 1) and attaches them to the handle; every ``accum_gradients*`` call then folds its
        forward's batch statistics in with momentum ``1 - bn_decay``, and ``set_bn_mode('moving')`` makes the forward-only
        calls normalise with them; ``set_bn_mode('frozen')`` also trains on them as constants (fine-tuning, no update of the buffer).
        False: nothing is allocated and every call does what it did without the keyword."""
        if not 0.0 <= float(bn_decay) <= 1.0:
            raise ValueError('bn_decay = %r outside [0, 1]' % (bn_decay,))
        self._bn_tracking = bool(bn_moving)
        self._bn_decay = float(bn_decay)
        self._bn_mode = 'batch'
        self._bn_buf = None
        if precision not in ('fp32', 'bf16'):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        self._precision = precision
        self._trainable = bool(trainable)
        self._use_weight = bool(use_weight)
        self._learning_rate = learning_rate
        self._bn_eps = float(bn_eps)

        self._data_size = int(np.prod(self._dims))
        self._label_size = int(np.prod(self._dims[:-1]))

        graph = Graph()
        shape_dim = tuple(int(d) for d in np.insert(self._dims, 0, -1))
        net = self._build(input_tensor=SymTensor(shape_dim, graph, 'input_prep/data_reshape'))
        if tuple(net.shape[1:]) != tuple(shape_dim[1:-1]) + (self._num_class,):
            raise ValueError('_build returned logits of shape %s' % (net.shape,))
        self._graph = graph

        self._softmax = None
        self._loss = None
        self._accuracy_allpix = None
        self._accuracy_nonzero = None
        self._merged_summary = None
        self._opt = None
        if self._trainable:
            # lib/ssnet.py:72-75: default AdamOptimizer() when learning_rate <= 0
            if self._learning_rate is None or self._learning_rate <= 0:
                self._opt = _Adam(0.001)
            else:
                self._opt = _Adam(self._learning_rate)

        self._cfg = self._native_config(max_batch=1)
        self._check_plan()
        if allocate:
            self._allocate(device, seed)

    def _native_config(self, max_batch):
        cfg = _lib.ursn_config()
        cfg.ndim = len(self._dims) - 1
        for i in range(3):
            cfg.spatial[i] = int(self._dims[i]) if i < cfg.ndim else 1
        cfg.cin = int(self._dims[-1])
        cfg.base_filters = int(getattr(self, '_base_num_outputs', 16))
        cfg.num_class = self._num_class
        cfg.num_strides = int(getattr(self, '_num_strides', 5))
        cfg.max_batch = int(max_batch)
        cfg.trainable = int(self._trainable)
        cfg.use_weight = int(self._use_weight)
        cfg.bn_eps = self._bn_eps
        cfg.act_dtype = 1 if getattr(self, '_precision', 'fp32') == 'bf16' else 0
        return cfg

    def _check_plan(self):
        """The native library implements the U-ResNet topology of lib/uresnet.py; a subclass whose
        ``_build`` records anything else cannot be executed (there is no generic graph executor).
        What ``_build`` recorded -- every conv-like layer's scope, kind, kernel, stride, channels and
        activation, and the operand order of every tf.concat -- is compared with the layer / concat
        tables of the plan the library compiles for this configuration (ursn_query_layer /
        ursn_query_concat), not with a second Python copy of the formula."""
        lib = _lib.load()
        if int(getattr(self, '_num_strides', 5)) > 5:
            # lib/uresnet.py:100 names the decoder units 'resnet_module%d' % (step + 5): with more than 5 strides they
            # collide with the encoder's scopes (TensorFlow raises on the duplicate variable scope as well)
            raise ValueError('num_strides > 5: decoder scope names collide with the encoder (lib/uresnet.py:100)')
        sizes = _lib.ursn_sizes()
        _lib.check(lib.ursn_query(ctypes.byref(self._cfg), ctypes.byref(sizes)))
        self._n_params = int(sizes.n_params)
        native = []
        info = _lib.ursn_layer_info()
        for i in range(int(sizes.n_layers)):
            _lib.check(lib.ursn_query_layer(ctypes.byref(self._cfg), i, ctypes.byref(info)))
            native.append(dict(name=info.name.decode(), kind='deconv' if info.transposed else 'conv', k=int(info.k),
                               stride=int(info.stride), cin=int(info.cin), cout=int(info.cout), relu=bool(info.relu),
                               w_offset=int(info.w_offset), beta_offset=int(info.beta_offset)))
        keys = ('name', 'kind', 'k', 'stride', 'cin', 'cout', 'relu')
        got = [tuple(l[k] for k in keys) for l in self._graph.layers]
        want = [tuple(l[k] for k in keys) for l in native]
        if got != want:
            diff = [(g, w) for g, w in zip(got, want) if g != w][:1] or [(len(got), len(want))]
            raise NotImplementedError('_build recorded a topology other than lib/uresnet.py:22-123 (first difference, '
                                      'recorded vs native plan: %r); only that hot path is implemented natively' % (diff[0],))
        a, b = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
        ns = int(getattr(self, '_num_strides', 5))
        native_cats = []
        for step in range(ns):
            _lib.check(lib.ursn_query_concat(ctypes.byref(self._cfg), step, a, b, 128))
            native_cats.append((a.value.decode(), b.value.decode()))
        if [(x, y) for (_, x, y) in self._graph.concats] != native_cats:
            raise NotImplementedError('_build concatenates %r; the native plan implements tf.concat([deconv_i, skip]) = %r '
                                      '(lib/uresnet.py:81)' % ([(x, y) for (_, x, y) in self._graph.concats], native_cats))
        names = [l['name'] for l in native]
        if len(set(names)) != len(names):
            raise ValueError('duplicate variable scopes in the plan')
        specs = []
        nd = len(self._dims) - 1
        for l in native:
            wshape = (l['k'],) * nd + ((l['cin'], l['cout']) if l['kind'] == 'conv' else (l['cout'], l['cin']))
            specs.append((l['name'] + '/weights', wshape, l['w_offset'], int(np.prod(wshape))))
            specs.append((l['name'] + '/BatchNorm/beta', (l['cout'],), l['beta_offset'], l['cout']))
        end = max(off + n for _, _, off, n in specs)
        if end != self._n_params or sum(n for _, _, _, n in specs) != self._n_params:
            raise RuntimeError('parameter table does not tile the flat buffer: %d vs native %d' % (end, self._n_params))
        self._specs = specs
        # moving statistics: per layer [moving_mean[cout] | moving_variance[cout]], unpadded, in this order (ursn_bn_attach)
        self._bn_specs, off = [], 0
        for l in native:
            self._bn_specs.append((l['name'] + '/BatchNorm', l['cout'], off))
            off += 2 * l['cout']
        total = ctypes.c_int64(0)
        _lib.check(lib.ursn_bn_moving_size(ctypes.byref(self._cfg), ctypes.byref(total)))
        if total.value != off:
            raise RuntimeError('moving-statistics table does not tile the buffer: %d vs native %d' % (off, total.value))
        self._bn_size = off

    # ------------------------------------------------------------------------------------------
    # device state
    # ------------------------------------------------------------------------------------------
    def _allocate(self, device, seed):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('ssnet_base.construct: no HIP device visible; the U-ResNet path has no CPU fallback '
                               '(pass allocate=False to only record/check the topology)')
        self._device = torch.device('cuda', torch.cuda.current_device() if device is None else int(device))
        n = self._n_params
        self._params = torch.empty(n, dtype=torch.float32, device=self._device)
        self._grads = self._adam_m = self._adam_v = None
        if self._trainable:
            self._grads = torch.zeros(n, dtype=torch.float32, device=self._device)
            self._adam_m = torch.zeros(n, dtype=torch.float32, device=self._device)
            self._adam_v = torch.zeros(n, dtype=torch.float32, device=self._device)
        if getattr(self, '_bn_tracking', False):
            self._bn_buf = torch.empty(self._bn_size, dtype=torch.float32, device=self._device)
            self.reset_bn_moving()
        self.initialize_variables(seed)

    def initialize_variables(self, seed=1234):
        """tf.global_variables_initializer (lib/ssnet_trainval.py:113): Xavier-uniform weights, beta = 0
        (SURVEY.md Appendix B-6).  TensorFlow's RNG stream is not reproduced."""
        import torch
        rng = np.random.default_rng(seed)
        host = np.zeros(self._n_params, np.float32)
        nd = len(self._dims) - 1
        for name, shape, off, n in self._specs:
            if name.endswith('/weights'):
                fan = int(np.prod(shape[:nd]))
                lim = math.sqrt(6.0 / (fan * (shape[-1] + shape[-2])))
                host[off:off + n] = rng.uniform(-lim, lim, size=n).astype(np.float32)
        self._params.copy_(torch.from_numpy(host))
        if self._trainable:
            self._adam_m.zero_(); self._adam_v.zero_(); self._grads.zero_()
        if self._handle is not None:
            _lib.check(_lib.load().ursn_set_adam_step(self._handle, 0))

    def _ensure_handle(self, batch):
        import torch
        if self._params is None:
            raise RuntimeError('construct(allocate=True) has not been called')
        if self._handle is not None and batch <= self._max_batch:
            return
        lib = _lib.load()
        step = 0
        if self._handle is not None:
            t = ctypes.c_int64(0)
            _lib.check(lib.ursn_get_adam_step(self._handle, ctypes.byref(t)))
            step = t.value
            self._opt_carry_counters()
            self._destroy()
        cfg = self._native_config(max_batch=batch)
        sizes = _lib.ursn_sizes()
        _lib.check(lib.ursn_query(ctypes.byref(cfg), ctypes.byref(sizes)))
        # activations of every layer stay resident for the backward pass (sized for 288 GB of HBM, no recomputation): say
        # so before the allocator raises something less readable
        self._workspace = None
        torch.cuda.empty_cache()
        free_b, total_b = torch.cuda.mem_get_info(self._device)
        if int(sizes.workspace_bytes) + (64 << 20) > free_b:
            raise MemoryError('U-ResNet workspace for batch %d needs %.1f GB but only %.1f of %.1f GB of HBM are free; '
                              'use a smaller MINIBATCH_SIZE with more NUM_MINIBATCHES (same gradient sum, '
                              'lib/ssnet.py:77)' % (batch, sizes.workspace_bytes / 1e9, free_b / 1e9, total_b / 1e9))
        self._workspace = torch.empty(int(sizes.workspace_bytes) + 256, dtype=torch.uint8, device=self._device)
        wptr = (self._workspace.data_ptr() + 255) & ~255
        h = ctypes.c_void_p()
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(lib.ursn_create(ctypes.byref(cfg), p(self._params), p(self._grads), p(self._adam_m),
                                   p(self._adam_v), ctypes.c_void_p(wptr), int(sizes.workspace_bytes),
                                   ctypes.byref(h)))
        self._handle, self._max_batch, self._cfg = h, batch, cfg
        _lib.check(lib.ursn_set_adam_step(self._handle, step))
        if getattr(self, '_bn_buf', None) is not None:   # caller-owned like the parameters: a new handle loses nothing
            _lib.check(lib.ursn_bn_attach(self._handle, p(self._bn_buf)))
            _lib.check(lib.ursn_bn_set_frozen(self._handle, int(self._bn_mode in ('moving', 'frozen'))))
            if self._bn_mode == 'frozen':
                _lib.check(lib.ursn_bn_frozen_train(self._handle, 1))
        if getattr(self, '_opt_state', None) is not None:   # caller-owned as well; attaching rebuilds the tables for this handle
            _lib.check(lib.ursn_opt_attach(self._handle, p(self._opt_state), self._opt_state.numel()))

    def _destroy(self):
        if getattr(self, '_handle', None) is not None:
            _lib.load().ursn_destroy(self._handle)
            self._handle = None
            self._workspace = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _stream(self, sess):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

    # ------------------------------------------------------------------------------------------
    # host feed (lib/ssnet.py:141-153 feed_dict; lib/ssnet_trainval.py:167-188 hands over IO buffers that are only
    # valid until the next io.next() and are mutated in place at :173)
    # ------------------------------------------------------------------------------------------
    class _FeedSlot(object):
        """One role's (data / label / weight) staging state: two device buffers used alternately, one pinned host
        buffer for callers that hand over pageable memory, and the events that order copy and compute."""
        __slots__ = ('dev', 'pinned', 'turn', 'consumed', 'copied')

        def __init__(self):
            self.dev, self.pinned, self.turn = [None, None], None, 0
            self.consumed = [None, None]   # recorded on the compute stream after the last launch that reads dev[i]
            self.copied = None

    def _copy_stream(self):
        import torch
        if getattr(self, '_h2d_stream', None) is None:
            self._h2d_stream = torch.cuda.Stream(device=self._device)
            self._feed_slots = {}
            self.feed_stats = {'h2d_bytes': 0, 'h2d_calls': 0, 'staged_bytes': 0}
        return self._h2d_stream

    def _feed(self, x, cols, what):
        """numpy / torch input [N, cols] -> contiguous fp32 device tensor.

        Host arrays travel on a dedicated copy stream from page-locked memory: directly from the caller's buffer when
        it already is page-locked (synthetic_threadio produces into pinned buffers), else through a pinned staging
        buffer.  The call returns once the COPY has completed (the caller may then reuse / mutate its buffer, as the
        reference's IO does), but it never waits for compute: with ``accum_gradients(fetch=False)`` the copy of
        minibatch k+1 overlaps the kernels of minibatch k.  Each role alternates between two device buffers; a buffer
        is only overwritten after the launch that last read it has finished (event recorded by ``_mark_consumed``)."""
        import torch
        if isinstance(x, torch.Tensor):
            if x.device == self._device and x.dtype == torch.float32 and x.is_contiguous():
                return x.reshape(-1, cols)
            if x.device.type != 'cpu':
                return x.to(device=self._device, dtype=torch.float32).reshape(-1, cols).contiguous()
            x = x.numpy()
        host = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, cols)
        n = host.shape[0]
        cs = self._copy_stream()
        slot = self._feed_slots.setdefault(what, ssnet_base._FeedSlot())
        i = slot.turn
        slot.turn ^= 1
        if slot.dev[i] is None or slot.dev[i].shape[0] < n:
            slot.dev[i] = torch.empty((n, cols), dtype=torch.float32, device=self._device)
            slot.consumed[i] = None
            # the caching allocator hands out blocks in compute-stream order: a block freed with kernels still pending on
            # the compute stream may come back here, and the copy stream must not write it before they have finished
            cs.wait_stream(torch.cuda.current_stream(self._device))
            slot.dev[i].record_stream(cs)
        dst = slot.dev[i][:n]
        src = torch.from_numpy(host)
        if not src.is_pinned():
            if slot.pinned is None or slot.pinned.shape[0] < n:
                slot.pinned = torch.empty((n, cols), dtype=torch.float32, pin_memory=True)
            if slot.copied is not None:
                slot.copied.synchronize()      # the previous copy out of the staging buffer
            slot.pinned[:n].copy_(src)
            src = slot.pinned[:n]
            self.feed_stats['staged_bytes'] += host.nbytes
        with torch.cuda.stream(cs):
            if slot.consumed[i] is not None:
                cs.wait_event(slot.consumed[i])
            dst.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        slot.copied = ev
        torch.cuda.current_stream(self._device).wait_event(ev)
        ev.synchronize()                       # copy only; kernels of earlier minibatches keep running
        self.feed_stats['h2d_bytes'] += host.nbytes
        self.feed_stats['h2d_calls'] += 1
        return dst

    def _mark_consumed(self, fd):
        """After the launches reading the fed tensors are queued: later copies into the same device buffers wait."""
        import torch
        slots = getattr(self, '_feed_slots', None)
        if not slots:
            return
        ev = None
        for t in fd.values():
            for slot in slots.values():
                for i in (0, 1):
                    if slot.dev[i] is not None and t.data_ptr() == slot.dev[i].data_ptr():
                        if ev is None:
                            ev = torch.cuda.Event()
                            ev.record(torch.cuda.current_stream(self._device))
                        slot.consumed[i] = ev

    # ------------------------------------------------------------------------------------------
    # per-event weight normalisation on the device (lib/ssnet_trainval.py:173,204 do it on the host)
    # ------------------------------------------------------------------------------------------
    def _normalize_fed_weight(self, fd, sess):
        """``fd['input_weight'] /= its per-event sums`` by ``ursn_normalize_weights`` on the compute stream, which ``_feed`` has
        already made wait for the copy.  A tensor in one of the net's own feed slots (the voxel expansion's dense weight buffer
        is one) is normalised in place; anything else is a caller's device tensor that ``_feed`` handed through, and is
        normalised into one of two private buffers used alternately, never written.  The caller's host array is never written
        either -- on purpose unlike the reference, which mutates its IO buffer.  ``fd`` then holds the normalised tensor, so
        whoever re-runs ``last_feed()`` passes ``normalize_weight=False``."""
        import torch
        w = fd.get('input_weight') if self._use_weight else None
        if w is None:
            return
        n, V = int(w.shape[0]), int(w.shape[1])
        lib = _lib.load()
        need = int(lib.ursn_normalize_weights_scratch_bytes(n, V))
        scratch = getattr(self, '_wnorm_scratch', None)
        if scratch is None or scratch.numel() * 8 < need:
            scratch = self._wnorm_scratch = torch.empty(max(need // 8, 1), dtype=torch.float64, device=self._device)
        own = any(d is not None and d.data_ptr() == w.data_ptr()
                  for slot in getattr(self, '_feed_slots', {}).values() for d in slot.dev)
        out = w
        if not own:
            bufs = getattr(self, '_wnorm_out', None)
            if bufs is None:
                bufs = self._wnorm_out = [None, None, 0]
            k = bufs[2]
            bufs[2] ^= 1
            if bufs[k] is None or bufs[k].numel() < n * V:
                bufs[k] = torch.empty(n * V, dtype=torch.float32, device=self._device)
            out = bufs[k][:n * V].view(n, V)
        _lib.check(lib.ursn_normalize_weights(self._ptr(w), self._ptr(out), n, V, None, self._ptr(scratch),
                                              scratch.numel() * 8, self._stream(sess)))
        fd['input_weight'] = out

    # ------------------------------------------------------------------------------------------
    # loss weights made on the device from the label (not in the reference, which reads them as a stored larcv product;
    # definition and numpy statement: weights.py)
    # ------------------------------------------------------------------------------------------
    def _check_make_weight(self, spec, given, what):
        """The refusals of ``make_weight=spec``, before anything touches the device."""
        from .weights import WeightSpec
        if not isinstance(spec, WeightSpec):
            raise ValueError('%s: make_weight = %r, expected a WeightSpec or None' % (what, spec))
        if given is not None:
            raise ValueError('%s: make_weight makes the weights on the device; a weight was given as well' % what)
        if not self._use_weight:
            raise ValueError('%s: make_weight needs a network constructed with use_weight=True' % what)
        spec.scales(self._num_class)

    def _make_fed_weight(self, fd, spec, sess, counts=None):
        """``fd['input_weight'] = ursn_make_weights(fd['input_label'])`` on the compute stream, into an alternating pair of feed
        slots registered like the voxel expansion's: ``_normalize_fed_weight`` then works in place, ``last_feed`` holds the weights
        and ``_mark_consumed`` covers them.  The scratch is cached on the object and grown on demand."""
        import torch
        self._copy_stream()                         # the slot table lives with the copy stream
        lab = fd['input_label']
        n, V = int(lab.shape[0]), int(lab.shape[1])
        lib, nd = _lib.load(), len(self._dims) - 1
        d = _lib.ursn_make_weights_desc()
        d.ndim, d.n, d.voxels, d.ncls, d.radius, d.mode = nd, n, V, self._num_class, spec.radius, spec.mode_code()
        for i in range(nd):
            d.spatial[i] = int(self._dims[i])
        for i, v in enumerate(spec.scales(self._num_class)):
            d.scale[i] = float(v)
        need = int(lib.ursn_make_weights_scratch_bytes(nd, d.spatial, n, d.ncls, d.radius))
        scratch = getattr(self, '_mkw_scratch', None)
        if scratch is None or scratch.numel() * 8 < need:
            scratch = self._mkw_scratch = torch.empty(max((need + 7) // 8, 1), dtype=torch.float64, device=self._device)
        slot = self._feed_slots.setdefault('made_weight', ssnet_base._FeedSlot())
        k = slot.turn
        slot.turn ^= 1
        if slot.dev[k] is None or slot.dev[k].shape[0] < n:
            slot.dev[k] = torch.empty((n, V), dtype=torch.float32, device=self._device)
            slot.consumed[k] = None
        out = slot.dev[k][:n]
        _lib.check(lib.ursn_make_weights(ctypes.byref(d), self._ptr(lab), self._ptr(out), self._ptr(counts), self._ptr(scratch),
                                         scratch.numel() * 8, self._stream(sess)))
        fd['input_weight'] = out

    def make_weights(self, sess, input_label, spec, as_numpy=False, with_counts=False):
        """The loss weights of ``spec`` (weights.WeightSpec) for ``input_label`` [N, voxels] (host array or device tensor), made on
        the device: a device tensor [N, voxels] (one of the net's own buffers, valid until two more batches have been made) or,
        with ``as_numpy``, a host array.  ``with_counts``: also ``counts`` int64 [N, num_class + 1], the voxels per category."""
        import torch
        from .weights import WeightSpec
        if not isinstance(spec, WeightSpec):
            raise ValueError('make_weights: spec = %r, expected a WeightSpec' % (spec,))
        spec.scales(self._num_class)
        if getattr(self, '_params', None) is None:
            raise RuntimeError('construct(allocate=True) has not been called')
        fd = {'input_label': self._feed(input_label, self._label_size, 'label')}
        n = int(fd['input_label'].shape[0])
        counts = torch.empty((n, self._num_class + 1), dtype=torch.int64, device=self._device) if with_counts else None
        self._make_fed_weight(fd, spec, sess, counts)
        self._mark_consumed({'input_label': fd['input_label']})
        w = fd['input_weight']
        if as_numpy:
            w = w.cpu().numpy()
        if not with_counts:
            return w
        return w, (counts.cpu().numpy() if as_numpy else counts)

    def _feed_for_made_weight(self, input_data, input_label):
        """``feed_dict`` without a weight role (the weights are made from the fed label)."""
        fd = {'input_data': self._feed(input_data, self._data_size, 'data'),
              'input_label': self._feed(input_label, self._label_size, 'label')}
        if fd['input_label'].shape[0] != fd['input_data'].shape[0]:
            raise ValueError('input_label has batch %d, input_data has %d' % (fd['input_label'].shape[0], fd['input_data'].shape[0]))
        return fd

    # ------------------------------------------------------------------------------------------
    # cube-symmetry augmentation and test-time averaging on the device (not in the reference, whose users flip and transpose
    # the volumes with numpy before the feed; codes and their numpy definition: symmetry.py)
    # ------------------------------------------------------------------------------------------
    def _sym_spatial(self):
        return (ctypes.c_int32 * 3)(*([int(d) for d in self._dims[:-1]] + [1])[:3])

    @staticmethod
    def _sym_ops(codes, n):
        """One code per event as the HOST int32 array the library reads; it validates the codes against the shape itself."""
        codes = [int(c) for c in codes]
        if len(codes) != n:
            raise ValueError('symmetry: %d codes for a batch of %d events' % (len(codes), n))
        return (ctypes.c_int32 * n)(*codes)

    def _sym_desc(self, ops, n, channels):
        d = _lib.ursn_sym_desc()
        d.ndim = len(self._dims) - 1
        for i in range(d.ndim):
            d.spatial[i] = int(self._dims[i])
        d.n, d.channels = n, channels
        d.ops = ctypes.cast(ops, ctypes.POINTER(ctypes.c_int32))
        return d

    def _apply_symmetry(self, fd, symmetry, sess):
        """``fd`` as ``_feed`` left it -> the same roles with event i under operation ``symmetry[i]``, written by ``ursn_sym_apply``
        on the compute stream (which ``_feed`` has made wait for the copies) into a second set of feed slots, two buffers per
        role used alternately and registered like the voxel expansion's, so ``last_feed``, ``_mark_consumed`` and the in-place
        weight normalisation treat them like fed tensors.  With one input channel the whole triple is ONE launch."""
        import torch
        self._copy_stream()                         # the slot table lives with the copy stream
        n = int(fd['input_data'].shape[0])
        ops = self._sym_ops(symmetry, n)
        out = {}
        for key, t in fd.items():
            ds = self._feed_slots.setdefault('sym_' + key[len('input_'):], ssnet_base._FeedSlot())
            k = ds.turn
            ds.turn ^= 1
            if ds.dev[k] is None or ds.dev[k].shape[0] < n:
                ds.dev[k] = torch.empty((n, int(t.shape[1])), dtype=torch.float32, device=self._device)
                ds.consumed[k] = None
            out[key] = ds.dev[k][:n]
        lib, cin = _lib.load(), int(self._dims[-1])
        rest = [k for k in ('input_label', 'input_weight') if k in fd]
        calls = [(cin, ['input_data'])] + ([(1, rest)] if rest else [])
        if cin == 1:
            calls = [(1, ['input_data'] + rest)]
        for channels, keys in calls:
            d = self._sym_desc(ops, n, channels)
            pairs = []
            for k in keys:
                pairs += [self._ptr(fd[k]), self._ptr(out[k])]
            pairs += [None] * (6 - len(pairs))
            _lib.check(lib.ursn_sym_apply(ctypes.byref(d), *(pairs + [self._stream(sess)])))
        self._mark_consumed(fd)                     # the copies' buffers are free once the permutation has read them
        return out

    def inference_tta(self, sess, input_data, codes, as_numpy=True):
        """Test-time averaging of ``inference`` over symmetric views: for each code of ``codes`` the data is permuted on the
        device (``ursn_sym_apply``), the forward pass and softmax run, and ``ursn_sym_accumulate`` maps the score volume back with
        the inverse code into one result buffer.  Returns ``mean_k inv_k(softmax_k)`` [N, *spatial, num_class], formed as an fp32
        left-to-right sum in list order and then multiplied by ``np.float32(1 / K)``; only the result crosses PCIe."""
        import torch
        from . import symmetry as S
        codes = [int(c) for c in codes]
        if not codes:
            raise ValueError('inference_tta: no codes')
        nd, K, C = len(self._dims) - 1, len(codes), self._num_class
        fd = {'input_data': self._feed(input_data, self._data_size, 'data')}
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        lib, stream = _lib.load(), self._stream(sess)
        view = torch.empty((n, self._data_size), dtype=torch.float32, device=self._device)
        sm = torch.empty((n,) + tuple(int(d) for d in self._dims[:-1]) + (C,), dtype=torch.float32, device=self._device)
        res = torch.empty_like(sm)
        out = (ctypes.c_float * 2)()
        for k, code in enumerate(codes):
            ops = self._sym_ops([code] * n, n)
            d = self._sym_desc(ops, n, int(self._dims[-1]))
            _lib.check(lib.ursn_sym_apply(ctypes.byref(d), self._ptr(fd['input_data']), self._ptr(view), None, None, None, None,
                                          stream))
            _lib.check(lib.ursn_infer(self._handle, self._ptr(view), None, n, self._ptr(sm), out, stream))
            back = self._sym_ops([S.inverse(nd, code)] * n, n)
            d = self._sym_desc(back, n, C)
            _lib.check(lib.ursn_sym_accumulate(ctypes.byref(d), self._ptr(sm), self._ptr(res), int(k == 0),
                                               float(np.float32(1.0 / K)) if k == K - 1 else 1.0, stream))
        self._mark_consumed(fd)
        return res.cpu().numpy() if as_numpy else res

    def inference_voxel_scores_tta(self, sess, voxels, codes):
        """``inference_voxel_scores`` averaged over symmetric views.  Each view is expanded from the list by
        ``ursn_voxels_to_dense_sym``; ``ursn_voxel_index_sym`` gives the (unsorted) positions of the event's own voxels inside the
        view and ``ursn_infer_voxels`` gathers the scores there, so entry m of every view belongs to the voxel entry m came in as
        and no volume has to be mapped back.  The scores [M, num_class] are averaged on the device (fp32 left-to-right sum in list
        order, then times ``np.float32(1 / K)``); ``pred`` is the lowest-index argmax and ``ana`` the reference's rule
        (lib/ssnet_trainval.py:285-287) on the averaged scores.  Nothing dense crosses PCIe.  Returns a dict of per-event lists
        ``index`` / ``scores`` / ``pred`` / ``ana`` like ``inference_voxel_scores``."""
        import torch
        self._require_single_channel('inference_voxel_scores_tta')
        codes = [int(c) for c in codes]
        if not codes:
            raise ValueError('inference_voxel_scores_tta: no codes')
        if self._num_class < 3:
            raise ValueError('inference_voxel_scores_tta: the ana label needs >= 3 classes (num_class = %d)' % self._num_class)
        lib, nd, K, C = _lib.load(), len(self._dims) - 1, len(codes), self._num_class
        n, off = voxels.n, voxels.offsets
        M = int(off[-1])
        remapped = torch.empty(max(M, 1), dtype=torch.int32, device=self._device)
        total = None
        for code in codes:
            fd = self._feed_voxels(voxels, with_label=False, with_weight=False, symmetry=[code] * n)
            self._ensure_handle(n)
            slot, turn, d_offsets, d_index = self._fed_list
            _lib.check(lib.ursn_voxel_index_sym(nd, self._sym_spatial(), n, self._sym_ops([code] * n, n), ctypes.c_void_p(d_offsets),
                                                ctypes.c_void_p(d_index), self._ptr(remapped), self._stream(sess)))
            scores = torch.empty((max(M, 1), C), dtype=torch.float32, device=self._device)
            _lib.check(lib.ursn_infer_voxels(self._handle, self._ptr(fd['input_data']), None, n, ctypes.c_void_p(d_offsets),
                                             self._ptr(remapped), M, self._ptr(scores), None, None, None, self._stream(sess)))
            self._last_feed = fd
            self._mark_consumed(fd)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self._device))
            slot.consumed[turn] = done             # offsets / index have been read: the list buffer is free again
            total = scores if total is None else total + scores
        avg = (total * float(np.float32(1.0 / K)))[:M]
        classes = torch.arange(C, device=self._device)
        pred = torch.where(avg == avg.max(dim=1, keepdim=True).values, classes, C).min(dim=1).values.to(torch.uint8)
        shower, track = avg[:, 1], avg[:, 2]
        rule = (shower > track).to(torch.uint8) + (track >= shower).to(torch.uint8) * 2
        ana = rule * (torch.from_numpy(voxels.value[:M]).to(self._device) > 1.0).to(torch.uint8)
        res = {'index': [voxels.index[off[i]:off[i + 1]].copy() for i in range(n)]}
        for name, t in (('scores', avg), ('pred', pred), ('ana', ana)):
            host = t.cpu().numpy()
            res[name] = [host[off[i]:off[i + 1]].copy() for i in range(n)]
        return res

    # ------------------------------------------------------------------------------------------
    # voxel-list feed (not in the reference: larcv fills dense arrays; see VoxelBatch)
    # ------------------------------------------------------------------------------------------
    def _require_single_channel(self, what):
        if int(self._dims[-1]) != 1:
            raise ValueError('%s: voxel lists carry one value per voxel, so dims[-1] must be 1 (dims = %s)'
                             % (what, [int(d) for d in self._dims]))

    def _feed_voxels(self, vb, with_label=True, with_weight=None, symmetry=None):
        """VoxelBatch -> the dense device tensors of ``feed_dict``, without the dense arrays ever crossing PCIe.

        Every array of the batch is packed into ONE page-locked staging buffer and travels in ONE copy on the copy stream,
        under the discipline of ``_feed``: two device buffers used alternately, a buffer overwritten only after the launch
        that last read it (``consumed``), the call returning once the copy is done (``copied``) and never waiting for compute.
        ``ursn_voxels_to_dense`` then expands the list on the compute stream into per-role device tensors (two sets,
        alternating, registered as feed slots so ``last_feed`` / ``_mark_consumed`` treat them like fed tensors).  With
        ``symmetry`` (one code per event, symmetry.py) ``ursn_voxels_to_dense_sym`` expands instead: every list entry is written at
        its image under the event's operation."""
        import torch
        self._require_single_channel('_feed_voxels')
        vb.validate()
        if vb.voxels != self._label_size:
            raise ValueError('VoxelBatch of %d voxels per event fed to a network of %d' % (vb.voxels, self._label_size))
        if with_weight is None:
            with_weight = self._use_weight
        if with_weight and vb.weight is None:
            sys.stderr.write('Network configured to use loss pixel-weighting. Cannot run w/ weight=None...\n')
            raise TypeError
        if with_label and vb.label is None:
            raise ValueError('_feed_voxels: the batch has no label list')
        n, V = vb.n, vb.voxels
        parts = [('offsets', vb.offsets), ('index', vb.index), ('value', vb.value)]
        if with_label:
            parts.append(('label', vb.label))
        if with_weight:
            parts += [('weight', vb.weight), ('bg_weight', vb.bg_weight)]
        at, nbytes = {}, 0
        for name, a in parts:                      # every section starts on a 16-byte boundary
            at[name] = nbytes
            nbytes += (a.nbytes + 15) & ~15
        nbytes = max(nbytes, 16)
        cs = self._copy_stream()
        cur = torch.cuda.current_stream(self._device)
        slot = self._feed_slots.setdefault('voxel_list', ssnet_base._FeedSlot())
        i = slot.turn
        slot.turn ^= 1
        if slot.dev[i] is None or slot.dev[i].numel() < nbytes:
            slot.dev[i] = torch.empty(nbytes + nbytes // 2, dtype=torch.uint8, device=self._device)
            slot.consumed[i] = None
            cs.wait_stream(cur)                    # as in _feed: the block may come back with kernels still pending on it
            slot.dev[i].record_stream(cs)
        if slot.pinned is None or slot.pinned.numel() < nbytes:
            slot.pinned = torch.empty(nbytes + nbytes // 2, dtype=torch.uint8, pin_memory=True)
        if slot.copied is not None:
            slot.copied.synchronize()              # the previous copy out of the staging buffer
        stage = slot.pinned.numpy()
        for name, a in parts:
            stage[at[name]:at[name] + a.nbytes] = a.view(np.uint8)
        dst = slot.dev[i][:nbytes]
        with torch.cuda.stream(cs):
            if slot.consumed[i] is not None:
                cs.wait_event(slot.consumed[i])
            dst.copy_(slot.pinned[:nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        slot.copied = ev
        cur.wait_event(ev)
        ev.synchronize()                           # copy only; kernels of earlier minibatches keep running
        self.feed_stats['h2d_bytes'] += nbytes
        self.feed_stats['h2d_calls'] += 1
        self.feed_stats['staged_bytes'] += nbytes

        base = dst.data_ptr()
        b = _lib.ursn_voxel_batch()
        b.n, b.voxels = n, V
        b.offsets, b.index, b.value = base + at['offsets'], base + at['index'], base + at['value']
        b.label = base + at['label'] if with_label else None
        b.weight = base + at['weight'] if with_weight else None
        b.bg_weight = base + at['bg_weight'] if with_weight else None
        fd = self._expand_voxel_list(b, with_label, with_weight, symmetry)
        done = torch.cuda.Event()
        done.record(cur)
        slot.consumed[i] = done                    # the list buffer is free once the expansion has read it
        # inference_voxel_scores reads offsets / index again after the forward pass and moves `consumed` behind its own launch
        self._fed_list = (slot, i, base + at['offsets'], base + at['index'])
        self._fed_value = base + at['value']       # the same buffer: read by the object-record passes under the same `consumed`
        self._fed_label = (dst, at['label'], vb.label.nbytes) if with_label else None    # ... and where the label list lies in it
        return fd

    def _expand_voxel_list(self, b, with_label, with_weight, symmetry=None):
        """A device-resident ``ursn_voxel_batch`` (``_feed_voxels``' copy, or a crop batch ``ursn_crop_write`` made) -> the dense
        device tensors of ``feed_dict``, expanded on the compute stream into per-role device tensors (two sets, alternating,
        registered as feed slots so ``last_feed`` / ``_mark_consumed`` treat them like fed tensors)."""
        import torch
        self._copy_stream()                         # the slot table lives with the copy stream
        n, V = int(b.n), int(b.voxels)
        fd, roles = {}, ['data'] + (['label'] if with_label else []) + (['weight'] if with_weight else [])
        for role in roles:
            ds = self._feed_slots.setdefault('voxel_' + role, ssnet_base._FeedSlot())
            k = ds.turn
            ds.turn ^= 1
            if ds.dev[k] is None or ds.dev[k].shape[0] < n:
                ds.dev[k] = torch.empty((n, V), dtype=torch.float32, device=self._device)
                ds.consumed[k] = None
            fd['input_' + role] = ds.dev[k][:n]
        if symmetry is None:
            _lib.check(_lib.load().ursn_voxels_to_dense(ctypes.byref(b), self._ptr(fd['input_data']),
                                                        self._ptr(fd.get('input_label')), self._ptr(fd.get('input_weight')),
                                                        self._stream(None)))
        else:
            _lib.check(_lib.load().ursn_voxels_to_dense_sym(ctypes.byref(b), len(self._dims) - 1, self._sym_spatial(),
                                                            self._sym_ops(symmetry, n), self._ptr(fd['input_data']),
                                                            self._ptr(fd.get('input_label')), self._ptr(fd.get('input_weight')),
                                                            self._stream(None)))
        return fd

    def accum_gradients_voxels(self, sess, voxels, fetch=True, normalize_weight=False, symmetry=None, make_weight=None, crop=None,
                               loss=None):
        """``accum_gradients`` fed a VoxelBatch: same fetch-set, same return structure.  ``normalize_weight``: the expanded dense
        weight tensor is normalised per event on the device (``_normalize_fed_weight``), the same definition of the sum as the
        dense feed's; ``voxels.weight`` / ``bg_weight`` are not written and ``VoxelBatch.normalize_weights`` is not needed.
        ``symmetry``: as in ``accum_gradients``; the operation is index arithmetic inside the expansion's scatter and the list
        is neither rewritten nor re-sorted.  ``make_weight``: as in ``accum_gradients``; ``voxels.weight`` / ``bg_weight`` must be
        None, only offsets, index, value and label travel, and the expansion has no weight role.  ``crop`` (crop training, see
        "tiling" below): ``(big_batch, boxes)`` with ``big_batch`` from ``upload_voxels`` and ``boxes`` a ``tiling.Boxes`` of the
        network's own size (``tiling.random_boxes``); ``voxels`` must then be None, the minibatch is one event per box, cut out of
        the resident large batch by ``ursn_crop_write`` and fed through the same expansion, so ``symmetry``, ``make_weight`` and
        ``normalize_weight`` compose as they do for a fed batch.  None: the call is made exactly as without the keyword.
        ``loss``: as in ``accum_gradients``; it comes last, on the tensors the other keywords left."""
        if not self._trainable:
            raise RuntimeError('accum_gradients_voxels: constructed with trainable=False')
        if crop is not None:
            voxels = self._crop_source(voxels, crop, 'accum_gradients_voxels')
        if make_weight is not None:
            self._check_make_weight(make_weight, voxels.weight, 'accum_gradients_voxels')
        self._require_single_channel('accum_gradients_voxels')
        feed = self._feed_voxels if crop is None else (lambda vb, **kw: self._feed_crop(vb, crop[1], sess, **kw))
        if make_weight is None:
            fd = feed(voxels, symmetry=symmetry)
        else:
            fd = feed(voxels, with_weight=False, symmetry=symmetry)
            self._make_fed_weight(fd, make_weight, sess)
        if normalize_weight:
            self._normalize_fed_weight(fd, sess)
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        out = (ctypes.c_float * 3)()
        w = fd.get('input_weight') if self._use_weight else None
        self._step_call(fd, w, n, out if fetch else None, sess, loss)
        self._bn_track(sess)
        self._last_feed = fd
        self._mark_consumed(fd)
        doc = ['', 'loss', 'acc. all', 'acc. nonzero']
        if not fetch:
            return None, doc
        return [None, float(out[0]), float(out[1]), float(out[2])], doc

    def run_test_voxels(self, sess, voxels, normalize_weight=False, make_weight=None, crop=None, loss=None):
        """``run_test`` fed a VoxelBatch (``normalize_weight`` / ``make_weight`` / ``crop`` as in ``accum_gradients_voxels``)."""
        if crop is not None:
            voxels = self._crop_source(voxels, crop, 'run_test_voxels')
        if make_weight is not None:
            self._check_make_weight(make_weight, voxels.weight, 'run_test_voxels')
        self._require_single_channel('run_test_voxels')
        feed = self._feed_voxels if crop is None else (lambda vb, **kw: self._feed_crop(vb, crop[1], sess, **kw))
        if make_weight is None:
            fd = feed(voxels)
        else:
            fd = feed(voxels, with_weight=False)
            self._make_fed_weight(fd, make_weight, sess)
        if normalize_weight:
            self._normalize_fed_weight(fd, sess)
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        out = (ctypes.c_float * 3)()
        w = fd.get('input_weight') if self._use_weight else None
        self._eval_call(fd, w, n, out, sess, loss)
        self._mark_consumed(fd)
        return [float(out[0]), float(out[1]), float(out[2])], ['loss', 'acc. all', 'acc. nonzero']

    def inference_voxels(self, sess, voxels, with_labels=True):
        """``inference_labels`` from a VoxelBatch to voxel sets: the label volume (lib/ssnet_trainval.py:285-287) stays on the
        device and ``ursn_labels_to_voxels`` keeps its non-zeros, what the reference stores through larcv.as_tensor3d
        (lib/ssnet_trainval.py:299-302).  Returns [list of (index int32[], class uint8[]) per event (, acc_all, acc_nonzero
        with ``with_labels``)]; only offsets, index, class and the two accuracies come back to the host."""
        import torch
        self._require_single_channel('inference_voxels')
        fd = self._feed_voxels(voxels, with_label=with_labels, with_weight=False)
        n, V = int(fd['input_data'].shape[0]), self._label_size
        self._ensure_handle(n)
        lib = _lib.load()
        labels = torch.empty((n, V), dtype=torch.float32, device=self._device)
        acc = (ctypes.c_float * 2)()
        _lib.check(lib.ursn_infer_labels(self._handle, self._ptr(fd['input_data']), self._ptr(fd.get('input_label')), n,
                                         self._ptr(labels), None, acc, self._stream(sess)))
        self._last_feed = fd
        self._mark_consumed(fd)
        # the label rule ends in "* (data > 1.0)" and every unlisted voxel holds 0: the host knows the exact upper bound
        res = [self.labels_to_voxel_sets(sess, labels, int(np.count_nonzero(voxels.value > 1.0)))]
        if with_labels:
            res += [float(acc[0]), float(acc[1])]
        return res

    def labels_to_voxel_sets(self, sess, labels, cap):
        """Device label volume [n, voxels] -> per-event (index int32[], class uint8[]) of its non-zeros (``ursn_labels_to_voxels``);
        ``cap`` bounds their number over the batch."""
        import torch
        lib = _lib.load()
        n, V = int(labels.shape[0]), self._label_size
        index = torch.empty(max(cap, 1), dtype=torch.int32, device=self._device)
        cls = torch.empty(max(cap, 1), dtype=torch.uint8, device=self._device)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=self._device)
        sbytes = int(lib.ursn_labels_to_voxels_scratch_bytes(n, V))
        scratch = torch.empty(sbytes, dtype=torch.uint8, device=self._device)
        _lib.check(lib.ursn_labels_to_voxels(self._ptr(labels), n, V, self._ptr(index), self._ptr(cls), cap, self._ptr(offsets),
                                             self._ptr(scratch), sbytes, self._stream(sess)))
        off = offsets.cpu().numpy()
        assert 0 <= int(off[-1]) <= cap, 'labels_to_voxels: %d non-zero labels, at most %d expected' % (int(off[-1]), cap)
        idx, cl = index[:int(off[-1])].cpu().numpy(), cls[:int(off[-1])].cpu().numpy()
        return [(idx[off[i]:off[i + 1]].copy(), cl[off[i]:off[i + 1]].copy()) for i in range(n)]

    def inference_voxel_scores(self, sess, voxels, with_labels=True, want=('scores', 'pred', 'ana')):
        """The output side of the voxel-list boundary: class scores, argmax class and ana label (lib/ssnet_trainval.py:285-287) AT
        THE VOXELS THE EVENT CAME IN AS, gathered on the device from conv2's stored logits by one ``ursn_infer_voxels`` call.  No
        dense softmax is written and nothing dense crosses PCIe in either direction: only the [M]-sized arrays (and the two
        accuracies) come back.  Returns a dict of per-event lists, split at ``offsets``: ``index`` int32 [m_i], ``scores`` float32
        [m_i, num_class] (the bits ``inference`` holds at those voxels), ``pred`` uint8 [m_i], ``ana`` uint8 [m_i] -- those named in
        ``want`` -- plus ``acc_all`` / ``acc_nonzero`` with ``with_labels`` (the dense head then runs without a softmax output;
        without labels it is not launched at all)."""
        import torch
        self._require_single_channel('inference_voxel_scores')
        want = tuple(want)
        spec = self._cluster_wanted(want)
        if not want or any(w not in ('scores', 'pred', 'ana') for w in want if spec is None or w != 'cluster'):
            raise ValueError("inference_voxel_scores: want = %r, expected a non-empty subset of %r" % (want, self._want_names()))
        if 'ana' in want and self._num_class < 3:
            raise ValueError('inference_voxel_scores: the ana label needs >= 3 classes (num_class = %d)' % self._num_class)
        matching = spec is not None and getattr(self, '_cluster_matching_on', False)
        if matching and (not with_labels or voxels.label is None):
            raise ValueError('inference_voxel_scores: cluster matching is on and the batch has no labels to cluster')
        fd = self._feed_voxels(voxels, with_label=with_labels, with_weight=False)
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        slot, turn, d_offsets, d_index = self._fed_list
        off = voxels.offsets
        M = int(off[-1])
        kinds = {'scores': ((max(M, 1), self._num_class), torch.float32), 'pred': ((max(M, 1),), torch.uint8),
                 'ana': ((max(M, 1),), torch.uint8)}
        made = [w for w in want if w != 'cluster'] + ([spec.on] if spec is not None and spec.on not in want else [])
        dev = {w: torch.empty(kinds[w][0], dtype=kinds[w][1], device=self._device) for w in made}
        acc = (ctypes.c_float * 2)()
        _lib.check(_lib.load().ursn_infer_voxels(self._handle, self._ptr(fd['input_data']), self._ptr(fd.get('input_label')), n,
                                                 ctypes.c_void_p(d_offsets), ctypes.c_void_p(d_index), M, self._ptr(dev.get('scores')),
                                                 self._ptr(dev.get('pred')), self._ptr(dev.get('ana')),
                                                 acc if with_labels else None, self._stream(sess)))
        self._last_feed = fd
        self._mark_consumed(fd)
        pending = None
        if spec is not None:                       # behind the gather head, on the list it read
            pending = self._enqueue_clusters(sess, d_offsets, d_index, dev[spec.on], n, M, self._dims[:-1], spec)
        sspec = getattr(self, '_cluster_split_spec', None) if pending is not None else None
        split, base = None, pending                # base: the clustering the records below run on
        if sspec is not None:                      # behind the cluster passes, same lists; no table can overflow at M rows
            split = self._enqueue_cluster_split(sess, d_offsets, d_index, pending[0].data_ptr(), pending[2],
                                                pending[0].data_ptr() + 8 * pending[3], pending[1], n, M, self._dims[:-1], sspec, M, M, M)
            if getattr(self, '_cluster_split_downstream', False):
                base = (split[0], split[3], split[8], max(M, 1), n, M)
        objects = None
        if pending is not None and getattr(self, '_cluster_features_on', False):   # behind the cluster passes, same lists
            objects = self._enqueue_cluster_features(sess, d_offsets, d_index, self._fed_value, base, self._dims[:-1])
        pspec = getattr(self, '_cluster_profile_spec', None) if pending is not None else None
        prof = None
        if pspec is not None:                      # behind the object records, which run for it in any case
            prof_objects = objects if objects is not None else \
                self._enqueue_cluster_features(sess, d_offsets, d_index, self._fed_value, base, self._dims[:-1])
            prof = self._enqueue_cluster_profile(sess, d_offsets, d_index, self._fed_value, base, prof_objects, self._dims[:-1],
                                                 pspec, self._profile_bin_cap(M, pspec))
        vspec = getattr(self, '_cluster_vertex_spec', None) if pending is not None else None
        vtx = None
        if vspec is not None:                      # behind the object records, which run for it in any case
            vtx_objects = objects if objects is not None else prof_objects if pspec is not None else \
                self._enqueue_cluster_features(sess, d_offsets, d_index, self._fed_value, base, self._dims[:-1])
            vtx = self._enqueue_cluster_vertices(sess, d_offsets, d_index, base, vtx_objects, base[1], self._dims[:-1], vspec,
                                                 M, self._vertex_inc_cap(M))
        cspec = getattr(self, '_cluster_chain_spec', None) if pending is not None else None
        chain = None
        if cspec is not None:                      # behind the object records, which run for it in any case
            chain_objects = objects if objects is not None else prof_objects if pspec is not None else \
                vtx_objects if vspec is not None else \
                self._enqueue_cluster_features(sess, d_offsets, d_index, self._fed_value, base, self._dims[:-1])
            chain = self._enqueue_cluster_chains(sess, d_offsets, d_index, base, chain_objects, base[1], self._dims[:-1],
                                                 cspec, M)
        nspec = getattr(self, '_cluster_cone_spec', None) if pending is not None else None
        cone = None
        if nspec is not None:                      # behind the object records, which run for it in any case
            cone_objects = objects if objects is not None else prof_objects if pspec is not None else \
                vtx_objects if vspec is not None else chain_objects if cspec is not None else \
                self._enqueue_cluster_features(sess, d_offsets, d_index, self._fed_value, base, self._dims[:-1])
            cone = self._enqueue_cluster_cones(sess, d_offsets, d_index, base, cone_objects, base[1], self._dims[:-1],
                                               nspec, M)
        truth = match = None
        if matching:                               # the TRUE classes under the same spec, then the match of the two id arrays
            buf, at, nbytes = self._fed_label
            truth = self._enqueue_clusters(sess, d_offsets, d_index, self._label_classes(buf[at:at + nbytes].view(torch.float32), M),
                                           n, M, self._dims[:-1], spec)
            match = self._enqueue_cluster_match(sess, d_offsets, pending, truth, self._fed_value, n, M, False)
        gspec = getattr(self, '_cluster_graph_spec', None) if pending is not None else None
        graph = None
        if gspec is not None:                      # behind the cluster passes, same lists
            graph = self._enqueue_cluster_graph(sess, d_offsets, d_index, self._fed_value, base[0], base[2], base[1], n, M,
                                                self._dims[:-1], gspec, M + 1024, True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self._device))
        slot.consumed[turn] = done                 # the gather head has read offsets / index: the list buffer is free again
        res = {'index': [voxels.index[off[i]:off[i + 1]].copy() for i in range(n)]}
        for w in want:
            if w == 'cluster':
                continue
            host = dev[w][:M].cpu().numpy()
            res[w] = [host[off[i]:off[i + 1]].copy() for i in range(n)]
        if pending is not None:
            res['cluster'], res['clusters'] = self._fetch_clusters(pending, off)
        if split is not None:
            res['split'] = self._fetch_cluster_split(split, off, [int(t['first'].size) for t in res['clusters']])
        src = res['split'] if base is not pending else res      # what the records below describe: the pieces or the components
        if objects is not None:
            res['objects'] = self._fetch_cluster_features(objects, src['clusters'])
        if match is not None:
            res['true_cluster'], res['true_clusters'] = self._fetch_clusters(truth, off)
            res['match'] = self._fetch_cluster_match(match, res['clusters'], res['true_clusters'])
        if graph is not None:
            res['graph'] = self._finish_cluster_graph(sess, graph, voxels, src, gspec, self._dims[:-1])
        if prof is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(prof_objects, src['clusters'])
            res['profiles'] = self._finish_cluster_profile(sess, prof, records, voxels, src, pspec, self._dims[:-1])
        if vtx is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(vtx_objects, src['clusters'])
            res['vertices'] = self._finish_cluster_vertices(sess, vtx, records, voxels, src, vspec, self._dims[:-1])
        if chain is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(chain_objects, src['clusters'])
            res['chains'] = self._fetch_cluster_chains(chain, records, off)
        if cone is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(cone_objects, src['clusters'])
            res['cones'] = self._fetch_cluster_cones(cone, records, off)
        if with_labels:
            res['acc_all'], res['acc_nonzero'] = float(acc[0]), float(acc[1])
        return res

    # ------------------------------------------------------------------------------------------
    # voxel clusters (not in the reference, whose users label the dense volume on the host; definition and numpy statement:
    # clusters.py, device passes: csrc/cluster.hip)
    # ------------------------------------------------------------------------------------------
    def set_clustering(self, spec):
        """A ``clusters.ClusterSpec`` makes ``'cluster'`` a legal member of ``want`` in ``inference_voxel_scores`` and
        ``inference_tiled_voxel_scores`` (their defaults do not change); None takes it away again.  With it wanted the class array
        ``spec.on`` is made on the device even when it is not itself wanted, the cluster passes are enqueued behind the gather head
        (tiled: behind the last scatter, on the stitched list in the large shape) and the result gains ``cluster`` (int32 [m_i] per
        event, -1 = no cluster) and ``clusters`` (per event a dict of ``first`` / ``size`` / ``cls``)."""
        from .clusters import ClusterSpec
        if spec is not None:
            if not isinstance(spec, ClusterSpec):
                raise ValueError('set_clustering: spec = %r, expected a clusters.ClusterSpec or None' % (spec,))
            spec.axes(len(self._dims) - 1)
            if spec.on == 'ana' and self._num_class < 3:
                raise ValueError('set_clustering: the ana label needs >= 3 classes (num_class = %d)' % self._num_class)
        self._cluster_spec = spec

    def _cluster_wanted(self, want):
        """The spec when ``'cluster'`` is wanted and one is set, else None (``'cluster'`` is then an unknown name like any other)."""
        spec = getattr(self, '_cluster_spec', None)
        return spec if spec is not None and 'cluster' in want else None

    def _want_names(self):
        """The legal members of ``want`` of the voxel-score calls: ``'cluster'`` only while a spec is set."""
        return ('scores', 'pred', 'ana') + (('cluster',) if getattr(self, '_cluster_spec', None) is not None else ())

    def _enqueue_clusters(self, sess, d_offsets, d_index, d_cls, n, M, shape, spec):
        """``ursn_cluster_voxels`` on device lists (raw pointers or tensors); enqueues only.  Returns what ``_fetch_clusters`` reads."""
        import torch
        lib = _lib.load()
        shape = [int(s) for s in shape]
        conn, _ = spec.axes(len(shape))
        need = int(lib.ursn_cluster_scratch_bytes(n, M))
        if need == 0:
            raise ValueError('clusters: %d events with %d list entries are out of domain' % (n, M))
        scratch = getattr(self, '_cluster_scratch_buf', None)
        if scratch is None or scratch.numel() * 8 < need:
            scratch = self._cluster_scratch_buf = torch.empty((need + 7) // 8, dtype=torch.int64, device=self._device)
        cap = max(M, 1)
        ints = torch.empty(3 * cap + n + 1, dtype=torch.int32, device=self._device)    # cluster | first | size | count | status
        tcls = torch.empty(cap, dtype=torch.uint8, device=self._device)
        toff = torch.empty(n + 1, dtype=torch.int64, device=self._device)
        ptr = lambda x: x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_desc()
        d.ndim, d.n, d.m_total = len(shape), n, M
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.cls = ptr(d_offsets), ptr(d_index), ptr(d_cls)
        d.connectivity, d.class_mask, d.same_class, d.min_size = conn, spec.class_mask(), int(spec.same_class), spec.min_size
        o = _lib.ursn_cluster_out()
        base = ints.data_ptr()
        o.cluster, o.first, o.size, o.count, o.status = base, base + 4 * cap, base + 8 * cap, base + 12 * cap, base + 12 * cap + 4 * n
        o.cls, o.table_offsets, o.cap = tcls.data_ptr(), toff.data_ptr(), M
        _lib.check(lib.ursn_cluster_voxels(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), scratch.numel() * 8,
                                           self._stream(sess)))
        return ints, tcls, toff, cap, n, M

    @staticmethod
    def _fetch_clusters(pending, off):
        """The [M]-sized ids and the per-cluster table as per-event lists; raises when a bounded device loop ran out."""
        ints, tcls, toff, cap, n, M = pending
        toff = toff.cpu().numpy()
        total = int(toff[-1])
        small = ints[3 * cap:].cpu().numpy()
        if int(small[n]) != 0:
            raise _lib.UrsnError('cluster_voxels: a bounded device loop ran out (status %d); the ids are not valid' % int(small[n]))
        assert 0 <= total <= M and np.array_equal(np.diff(toff), small[:n]), 'cluster_voxels: table offsets and counts disagree'
        cluster = ints[:M].cpu().numpy()
        first, size = ints[cap:cap + total].cpu().numpy(), ints[2 * cap:2 * cap + total].cpu().numpy()
        cls = tcls[:total].cpu().numpy()
        per_event = [cluster[off[i]:off[i + 1]].copy() for i in range(n)]
        tables = [{'first': first[toff[i]:toff[i + 1]].copy(), 'size': size[toff[i]:toff[i + 1]].copy(),
                   'cls': cls[toff[i]:toff[i + 1]].copy()} for i in range(n)]
        return per_event, tables

    def cluster_voxels(self, sess, voxels_or_lists, cls, spec, shape=None):
        """Clusters of any per-event index lists and classes: ``voxels_or_lists`` is a VoxelBatch or a list of sorted per-event
        index arrays, ``cls`` the classes as one flat array or per-event arrays (the ``pred`` / ``ana`` lists of
        ``inference_voxel_scores_tta``, or true labels for a comparison against truth), ``shape`` the spatial shape the indices are
        row-major in (None: the network's).  Returns ``{'cluster': [...], 'clusters': [...]}`` as ``set_clustering`` describes."""
        import torch
        from .clusters import ClusterSpec
        if not isinstance(spec, ClusterSpec):
            raise ValueError('cluster_voxels: spec = %r, expected a clusters.ClusterSpec' % (spec,))
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        spec.axes(len(shape))
        if any(s < 1 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_voxels: shape = %r, expected extents >= 1 with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, VoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_voxels: %d events outside [1, 65535]' % n)
        if isinstance(cls, (list, tuple)):
            cls = np.concatenate([np.asarray(c).reshape(-1) for c in cls]) if len(cls) else np.zeros(0, np.uint8)
        cls = np.asarray(cls).reshape(-1)
        if cls.size != M or index.size != M:
            raise ValueError('cluster_voxels: %d list entries, %d indices, %d classes' % (M, index.size, cls.size))
        if M and (cls.min() < 0 or cls.max() > 255 or not np.array_equal(cls, cls.astype(np.uint8))):
            raise ValueError('cluster_voxels: classes must be integers in [0, 255]')
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self._device)
        d_off, d_index, d_cls = up(off, np.int64), up(index, np.int32), up(cls, np.uint8)
        pending = self._enqueue_clusters(sess, d_off, d_index, d_cls, n, M, shape, spec)
        cluster, tables = self._fetch_clusters(pending, off)
        return {'cluster': cluster, 'clusters': tables}

    # ------------------------------------------------------------------------------------------
    # per-cluster object records (definition and numpy statement: clusters.cluster_features_numpy, device passes:
    # csrc/cluster_features.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_features(self, on):
        """While on, and a cluster spec is set, and ``'cluster'`` is wanted, ``inference_voxel_scores`` and
        ``inference_tiled_voxel_scores`` enqueue ``ursn_cluster_features`` behind the cluster passes (tiled: on the stitched list in
        the large shape), with the batch's own resident value list, and the result gains ``objects``: per event a dict of arrays with
        one row per cluster (the fields of ``clusters.cluster_features_numpy`` plus ``first`` / ``size`` / ``cls`` of the cluster
        table).  The legal members of ``want`` do not change; never called, the results have the keys they had."""
        if type(on) is not bool:
            raise ValueError('set_cluster_features: on = %r, expected a bool' % (on,))
        self._cluster_features_on = on

    def _enqueue_cluster_features(self, sess, d_offsets, d_index, d_value, pending, shape):
        """``ursn_cluster_features`` behind ``_enqueue_clusters`` (its ids and table offsets stay on the device); enqueues only."""
        import torch
        lib = _lib.load()
        ints, _, toff, _, n, M = pending
        shape = [int(s) for s in shape]
        cap = M
        need = int(lib.ursn_cluster_features_scratch_bytes(n, M, cap))
        if need == 0:
            raise ValueError('cluster_features: %d events with %d list entries are out of domain' % (n, M))
        scratch = torch.empty(need // 8, dtype=torch.int64, device=self._device)
        itab = torch.empty((max(cap, 1), _lib.CLFEAT_I), dtype=torch.int64, device=self._device)
        rtab = torch.empty((max(cap, 1), _lib.CLFEAT_R), dtype=torch.float64, device=self._device)
        status = torch.empty(1, dtype=torch.int32, device=self._device)
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_feat_desc()
        d.ndim, d.n, d.m_total = len(shape), n, M
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.value, d.cluster, d.table_offsets = ptr(d_offsets), ptr(d_index), ptr(d_value), ints.data_ptr(), \
            toff.data_ptr()
        o = _lib.ursn_cluster_feat_out()
        o.itab, o.rtab, o.cap, o.status = itab.data_ptr(), rtab.data_ptr(), cap, status.data_ptr()
        _lib.check(lib.ursn_cluster_features(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, itab, rtab, status):
            t.record_stream(cur)
        return itab, rtab, status

    @staticmethod
    def _fetch_cluster_features(objects, tables):
        """The two object tables as per-event dicts of named arrays, joined with the cluster table's ``first`` / ``size`` / ``cls``."""
        itab, rtab, status = objects
        counts = [int(t['first'].size) for t in tables]
        total = int(sum(counts))
        code = int(status.cpu().numpy()[0])
        if code != 0:
            raise _lib.UrsnError('cluster_features: the ids, table offsets and lists disagree (status %d)' % code)
        assert total <= itab.shape[0], 'cluster_features: %d clusters, %d rows' % (total, itab.shape[0])
        it, rt = itab[:total].cpu().numpy(), rtab[:total].cpu().numpy()
        res, at = [], 0
        for t, k in zip(tables, counts):
            i, r = it[at:at + k], rt[at:at + k]
            at += k
            ev = {'n': i[:, 0].copy(), 'charge': i[:, 1].copy(), 's': i[:, 2:5].copy(), 'lo': i[:, 5:8].copy(),
                  'hi': i[:, 8:11].copy(), 'm': i[:, 11:14].copy(), 'd': i[:, 14:17].copy(), 'dd': i[:, 17:23].copy(),
                  'flags': i[:, 23].copy(), 'end_lo': i[:, 24].copy(), 'end_hi': i[:, 25].copy(),
                  'centroid': r[:, 0:3].copy(), 'cov': r[:, 3:9].copy(), 'eval': r[:, 9:12].copy(), 'axis': r[:, 12:15].copy(),
                  'length': r[:, 15].copy(), 't_lo': r[:, 16].astype(np.float32), 't_hi': r[:, 17].astype(np.float32),
                  'first': t['first'].copy(), 'size': t['size'].copy(), 'cls': t['cls'].copy()}
            assert np.array_equal(ev['n'], ev['size']), 'cluster_features: member counts and the cluster table disagree'
            res.append(ev)
        return res

    def cluster_features(self, sess, voxels_or_lists, value, clusters, shape=None):
        """Object records of clusters already made: ``voxels_or_lists`` and ``shape`` as ``cluster_voxels`` took them, ``value`` the
        entries' values as one flat array or per-event arrays (None: a VoxelBatch's own, or no charge for plain lists), ``clusters``
        the dict ``cluster_voxels`` returned.  Returns per event a dict of arrays with one row per cluster: the fields of
        ``clusters.cluster_features_numpy`` (``end_lo`` / ``end_hi`` are positions in the concatenated list) plus ``first`` /
        ``size`` / ``cls``."""
        import torch
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        if len(shape) not in (2, 3) or any(not 1 <= s <= 32768 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_features: shape = %r, expected 2 or 3 extents in [1, 32768] with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, VoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = voxels_or_lists.value
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_features: %d events outside [1, 65535]' % n)
        if isinstance(value, (list, tuple)):
            value = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in value]) if len(value) else np.zeros(0, np.float32)
        if value is not None:
            value = np.asarray(value, np.float32).reshape(-1)
        ids, tables = clusters['cluster'], clusters['clusters']
        if len(ids) != n or len(tables) != n:
            raise ValueError('cluster_features: %d events, clusters of %d / %d' % (n, len(ids), len(tables)))
        cluster = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in ids]) if n else np.zeros(0, np.int32)
        if cluster.size != M or index.size != M or (value is not None and value.size != M):
            raise ValueError('cluster_features: %d list entries, %d indices, %d ids, %s values'
                             % (M, index.size, cluster.size, 'no' if value is None else value.size))
        toff = np.concatenate([[0], np.cumsum([int(t['first'].size) for t in tables])]).astype(np.int64)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self._device)
        d_off, d_index, d_toff = up(off, np.int64), up(index, np.int32), up(toff, np.int64)
        d_cluster = up(cluster if M else np.zeros(1, np.int32), np.int32)
        d_value = None if value is None else up(value if M else np.zeros(1, np.float32), np.float32)
        objects = self._enqueue_cluster_features(sess, d_off, d_index, d_value, (d_cluster, None, d_toff, M, n, M), shape)
        return self._fetch_cluster_features(objects, tables)

    # ------------------------------------------------------------------------------------------
    # per-cluster charge profiles along the principal axis (definition and numpy statement: clusters.cluster_profile_numpy, device
    # passes: csrc/cluster_profile.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_profiles(self, spec):
        """A ``clusters.ClusterProfileSpec``: while one is set, and a cluster spec is set, and ``'cluster'`` is wanted,
        ``inference_voxel_scores`` and ``inference_tiled_voxel_scores`` enqueue ``ursn_cluster_profile`` behind the cluster passes
        and the object records (which run for it whether or not ``set_cluster_features`` is on; tiled: on the stitched list in the
        large shape), and the result gains ``profiles``: per event what ``cluster_profiles`` returns.  The row count is not known
        on the host there, so the bin table is sized from the list length alone: ``int(M * (1.75 / step + 1)) + 1`` bins -- a
        connected cluster of n members is at most sqrt(3) (n - 1) long (1.75 covers the fp32 rounding of the two end projections),
        so it has at most 1.75 (n - 1) / step + 1 bins.  Ids that are not connected clusters can exceed it; the device then reports
        the overflow and the result is made again by ``cluster_profiles`` on the returned ids, which sizes the table exactly.
        None switches it off.  The legal members of ``want`` do not change; never called, the results have the keys they had."""
        from .clusters import ClusterProfileSpec
        if spec is not None and not isinstance(spec, ClusterProfileSpec):
            raise ValueError('set_cluster_profiles: spec = %r, expected a clusters.ClusterProfileSpec or None' % (spec,))
        self._cluster_profile_spec = spec

    @staticmethod
    def _profile_bin_cap(M, spec):
        """Bins enough for every connected cluster of a list of ``M`` entries (``set_cluster_profiles`` has the reasoning)."""
        return min(int(M * (1.75 / spec.step + 1.0)) + 1, 2 ** 31 - 1)

    def _enqueue_cluster_profile(self, sess, d_offsets, d_index, d_value, pending, objects, shape, spec, bin_cap):
        """``ursn_cluster_profile`` behind ``_enqueue_cluster_features`` (whose tables stay on the device); enqueues only."""
        import torch
        lib = _lib.load()
        ints, _, toff, _, n, M = pending
        itab, rtab, _ = objects
        shape = [int(s) for s in shape]
        cap_rows, bin_cap = M, int(bin_cap)
        need = int(lib.ursn_cluster_profile_scratch_bytes(n, M, cap_rows, bin_cap))
        if need == 0:
            raise ValueError('cluster_profiles: %d events with %d list entries and %d bins are out of domain' % (n, M, bin_cap))
        scratch = torch.empty(need // 8, dtype=torch.int64, device=self._device)
        boff = torch.empty(cap_rows + 1, dtype=torch.int64, device=self._device)
        bi = torch.empty((max(bin_cap, 1), _lib.CLPROF_BI), dtype=torch.int64, device=self._device)
        br = torch.empty((max(bin_cap, 1), _lib.CLPROF_BR), dtype=torch.float64, device=self._device)
        ri = torch.empty((max(cap_rows, 1), _lib.CLPROF_RI), dtype=torch.int64, device=self._device)
        rr = torch.empty((max(cap_rows, 1), _lib.CLPROF_RR), dtype=torch.float64, device=self._device)
        status = torch.empty(1, dtype=torch.int32, device=self._device)
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_prof_desc()
        d.ndim, d.n, d.m_total = len(shape), n, M
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.value, d.cluster, d.table_offsets = ptr(d_offsets), ptr(d_index), ptr(d_value), ints.data_ptr(), \
            toff.data_ptr()
        d.itab, d.rtab, d.feat_cap = itab.data_ptr(), rtab.data_ptr(), M
        d.step, d.end_bins, d.max_bins = spec.step, spec.end_bins, spec.max_bins
        o = _lib.ursn_cluster_prof_out()
        o.bin_offsets, o.bin_itab, o.bin_rtab, o.row_itab, o.row_rtab = boff.data_ptr(), bi.data_ptr(), br.data_ptr(), \
            ri.data_ptr(), rr.data_ptr()
        o.cap_rows, o.bin_cap, o.status = cap_rows, bin_cap, status.data_ptr()
        _lib.check(lib.ursn_cluster_profile(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, boff, bi, br, ri, rr, status, itab, rtab):
            t.record_stream(cur)
        return boff, bi, br, ri, rr, status, bin_cap

    @staticmethod
    def _fetch_cluster_profile(prof, objects):
        """The profile tables as per-event dicts (``objects``: what ``_fetch_cluster_features`` returned for the same rows), or None
        when the bin table was too small."""
        from .clusters import PROFILE_BIN_INT, PROFILE_BIN_REAL, PROFILE_ROW_INT, PROFILE_ROW_REAL
        boff, bi, br, ri, rr, status, bin_cap = prof
        code = int(status.cpu().numpy()[0])
        if code & _lib.CLPROF_BIN_OVERFLOW:
            return None
        if code != 0:
            raise _lib.UrsnError('cluster_profile: the ids, table offsets, lists and object records disagree (status %d)' % code)
        counts = [int(o['n'].shape[0]) for o in objects]
        total = int(sum(counts))
        off = boff[:total + 1].cpu().numpy()
        B = int(off[-1])
        assert off[0] == 0 and B <= bin_cap, 'cluster_profile: %d bins, %d in the table' % (B, bin_cap)
        bi, br, ri, rr = bi[:B].cpu().numpy(), br[:B].cpu().numpy(), ri[:total].cpu().numpy(), rr[:total].cpu().numpy()
        res, at = [], 0
        for o, k in zip(objects, counts):
            lo, hi = int(off[at]), int(off[at + k])
            bins = {name: bi[lo:hi, c].copy() for c, name in enumerate(PROFILE_BIN_INT)}
            bins.update({name: br[lo:hi, c].copy() for c, name in enumerate(PROFILE_BIN_REAL)})
            rows = {name: ri[at:at + k, c].copy() for c, name in enumerate(PROFILE_ROW_INT)}
            rows.update({name: rr[at:at + k, c].copy() for c, name in enumerate(PROFILE_ROW_REAL)})
            res.append({'objects': o, 'rows': rows, 'bins': bins, 'bin_offsets': off[at:at + k + 1] - off[at]})
            at += k
        return res

    def _finish_cluster_profile(self, sess, prof, objects, voxels_or_lists, res, spec, shape, value=None):
        """The profiles enqueued with a voxel-score call, or -- the bin table was too small -- ``cluster_profiles`` on the
        returned ids."""
        got = self._fetch_cluster_profile(prof, objects)
        if got is None:
            got = self.cluster_profiles(sess, voxels_or_lists, value() if callable(value) else value, res, spec, shape=shape)
        return got

    def cluster_profiles(self, sess, voxels_or_lists, value, clusters, spec, shape=None):
        """Charge profiles of clusters already made: ``voxels_or_lists``, ``value``, ``clusters`` and ``shape`` as
        ``cluster_features`` takes them, ``spec`` a ``clusters.ClusterProfileSpec``.  Runs the object records, reads their
        ``length`` back, sizes the bin table exactly from it (``clusters.profile_bin_count``: the fp64 expression the device
        evaluates) and runs the profile.  Returns per event a dict: ``objects`` (as ``cluster_features``), ``rows`` (named columns
        ``clusters.PROFILE_ROW_INT`` / ``PROFILE_ROW_REAL``, one row per cluster), ``bins`` (``PROFILE_BIN_INT`` /
        ``PROFILE_BIN_REAL``, one row per bin) and ``bin_offsets`` [K_i + 1], event-local: the bins of cluster k are
        ``bin_offsets[k] .. bin_offsets[k + 1]``.  ``rows['direction']`` is the sign of the charge asymmetry between the two ends
        and nothing more."""
        import torch
        from .clusters import ClusterProfileSpec
        if not isinstance(spec, ClusterProfileSpec):
            raise ValueError('cluster_profiles: spec = %r, expected a clusters.ClusterProfileSpec' % (spec,))
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        if len(shape) not in (2, 3) or any(not 1 <= s <= 32768 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_profiles: shape = %r, expected 2 or 3 extents in [1, 32768] with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, VoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = voxels_or_lists.value
        elif isinstance(voxels_or_lists, _DeviceVoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = self._resident_value(voxels_or_lists)
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_profiles: %d events outside [1, 65535]' % n)
        if isinstance(value, (list, tuple)):
            value = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in value]) if len(value) else np.zeros(0, np.float32)
        if value is not None:
            value = np.asarray(value, np.float32).reshape(-1)
        ids, tables = clusters['cluster'], clusters['clusters']
        if len(ids) != n or len(tables) != n:
            raise ValueError('cluster_profiles: %d events, clusters of %d / %d' % (n, len(ids), len(tables)))
        cluster = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in ids]) if n else np.zeros(0, np.int32)
        if cluster.size != M or index.size != M or (value is not None and value.size != M):
            raise ValueError('cluster_profiles: %d list entries, %d indices, %d ids, %s values'
                             % (M, index.size, cluster.size, 'no' if value is None else value.size))
        toff = np.concatenate([[0], np.cumsum([int(t['first'].size) for t in tables])]).astype(np.int64)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self._device)
        d_off, d_index, d_toff = up(off, np.int64), up(index, np.int32), up(toff, np.int64)
        d_cluster = up(cluster if M else np.zeros(1, np.int32), np.int32)
        d_value = None if value is None else up(value if M else np.zeros(1, np.float32), np.float32)
        pending = (d_cluster, None, d_toff, M, n, M)
        dev_objects = self._enqueue_cluster_features(sess, d_off, d_index, d_value, pending, shape)
        objects = self._fetch_cluster_features(dev_objects, tables)
        from .clusters import profile_bin_count
        bin_cap = sum(profile_bin_count(length, spec.step, spec.max_bins)[0] for o in objects for length in o['length'])
        prof = self._enqueue_cluster_profile(sess, d_off, d_index, d_value, pending, dev_objects, shape, spec, bin_cap)
        got = self._fetch_cluster_profile(prof, objects)
        assert got is not None, 'cluster_profile: %d bins sized from the returned lengths were not enough' % bin_cap
        return got

    # ------------------------------------------------------------------------------------------
    # vertex candidates: where cluster end points meet (definition and numpy statement: clusters.cluster_vertices_numpy, device
    # passes: csrc/cluster_vertex.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_vertices(self, spec):
        """A ``clusters.ClusterVertexSpec``: while one is set, and a cluster spec is set, and ``'cluster'`` is wanted,
        ``inference_voxel_scores`` and ``inference_tiled_voxel_scores`` enqueue ``ursn_cluster_vertices`` behind the cluster passes
        and the object records (which run for it whether or not ``set_cluster_features`` is on; tiled: on the stitched list in the
        large shape, so a vertex can join ends from two tiles), and the result gains ``vertices``: per event what
        ``cluster_vertices`` returns.  The row count is not known on the host there, so the incidence table is sized from the list
        length; when the device reports more distinct incidences the result is made again by ``cluster_vertices`` on the returned
        ids.  Memory: with the row count unknown, the tables are laid out for ``M`` rows of a list of ``M`` entries -- 2 M vertex
        records, 4 M + 1024 incidences and the scratch for both, 1.1 to 1.4 KB of device memory per list entry for the duration of
        the call (4 to 5 GB for a list of 3.5 M entries); ``cluster_vertices`` on returned ids sizes them from the row count instead.
        None switches it off.  The legal members of ``want`` do not change; never called, the results have the keys they had."""
        from .clusters import ClusterVertexSpec
        if spec is not None and not isinstance(spec, ClusterVertexSpec):
            raise ValueError('set_cluster_vertices: spec = %r, expected a clusters.ClusterVertexSpec or None' % (spec,))
        self._cluster_vertex_spec = spec

    @staticmethod
    def _vertex_inc_cap(K):
        """The first incidence table for ``K`` rows: an end point mostly meets its own row and a few others."""
        return min(4 * K + 1024, 2 ** 30 - 1)

    def _enqueue_cluster_vertices(self, sess, d_offsets, d_index, pending, objects, d_cls, shape, spec, rows, inc_cap):
        """``ursn_cluster_vertices`` behind ``_enqueue_cluster_features`` (whose tables stay on the device); ``rows`` bounds the
        cluster rows (the list length when the count is still on the device); enqueues only."""
        import torch
        lib = _lib.load()
        ints, _, toff, _, n, M = pending
        itab, rtab, _ = objects
        shape = [int(s) for s in shape]
        rows, inc_cap = int(rows), int(inc_cap)
        need = int(lib.ursn_cluster_vertices_scratch_bytes(n, M, inc_cap))
        if need == 0:
            raise ValueError('cluster_vertices: %d events with %d list entries and %d incidences are out of domain' % (n, M, inc_cap))
        cap_v = 2 * rows
        scratch = torch.empty(need // 8, dtype=torch.int64, device=self._device)
        voff = torch.empty(n + 1, dtype=torch.int64, device=self._device)
        ioff = torch.empty(cap_v + 1, dtype=torch.int64, device=self._device)
        vi = torch.empty((max(cap_v, 1), _lib.CLVTX_VI), dtype=torch.int64, device=self._device)
        vr = torch.empty((max(cap_v, 1), _lib.CLVTX_VR), dtype=torch.float64, device=self._device)
        inc = torch.empty((max(inc_cap, 1), _lib.CLVTX_IN), dtype=torch.int64, device=self._device)
        rv = torch.empty((max(rows, 1), 2), dtype=torch.int32, device=self._device)
        ev = torch.empty((n, _lib.CLVTX_EV), dtype=torch.int64, device=self._device)
        status = torch.empty(1, dtype=torch.int32, device=self._device)
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_vtx_desc()
        d.ndim, d.n, d.m_total, d.radius, d.inc_cap = len(shape), n, M, spec.radius, inc_cap
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.cluster, d.table_offsets = ptr(d_offsets), ptr(d_index), ints.data_ptr(), toff.data_ptr()
        d.itab, d.rtab, d.feat_cap, d.cls = itab.data_ptr(), rtab.data_ptr(), M, ptr(d_cls)
        d.min_size, d.class_mask = spec.min_size, spec.class_mask()
        o = _lib.ursn_cluster_vtx_out()
        o.vertex_offsets, o.vtx_itab, o.vtx_rtab, o.cap_vertices = voff.data_ptr(), vi.data_ptr(), vr.data_ptr(), cap_v
        o.inc_offsets, o.incidence, o.inc_out_cap = ioff.data_ptr(), inc.data_ptr(), inc_cap
        o.row_vertex, o.cap_rows, o.event, o.status = rv.data_ptr(), rows, ev.data_ptr(), status.data_ptr()
        _lib.check(lib.ursn_cluster_vertices(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, voff, ioff, vi, vr, inc, rv, ev, status, itab, rtab) + (() if d_cls is None else (d_cls,)):
            t.record_stream(cur)
        return voff, ioff, vi, vr, inc, rv, ev, status

    @staticmethod
    def _fetch_cluster_vertices(vtx, objects):
        """The vertex tables as per-event dicts (``objects``: what ``_fetch_cluster_features`` returned for the same rows), or None
        when the incidence table was too small."""
        from .clusters import VERTEX_EVENT, VERTEX_INT, VERTEX_REAL
        voff, ioff, vi, vr, inc, rv, ev, status = vtx
        code = int(status.cpu().numpy()[0])
        if code & _lib.CLVTX_INC_OVERFLOW:
            return None
        if code != 0:
            raise _lib.UrsnError('cluster_vertices: the ids, table offsets, lists and object records disagree (status %d)' % code)
        counts = [int(o['n'].shape[0]) for o in objects]
        voff = voff.cpu().numpy()
        V = int(voff[-1])
        assert voff[0] == 0 and V <= vi.shape[0] and sum(counts) <= rv.shape[0], 'cluster_vertices: %d vertices, %d in the table' % (
            V, vi.shape[0])
        ioff = ioff[:V + 1].cpu().numpy()
        total = int(ioff[-1])
        assert ioff[0] == 0 and total <= inc.shape[0], 'cluster_vertices: %d incidences, %d in the table' % (total, inc.shape[0])
        vi, vr, inc = vi[:V].cpu().numpy(), vr[:V].cpu().numpy(), inc[:total].cpu().numpy()
        rv, ev = rv[:sum(counts)].cpu().numpy(), ev.cpu().numpy()
        res, at = [], 0
        for i, (o, k) in enumerate(zip(objects, counts)):
            lo, hi = int(voff[i]), int(voff[i + 1])
            cols = {name: vi[lo:hi, c].copy() for c, name in enumerate(VERTEX_INT)}
            cols.update({name: vr[lo:hi, c].copy() for c, name in enumerate(VERTEX_REAL)})
            res.append({'objects': o, 'vertices': cols, 'incidence': inc[int(ioff[lo]):int(ioff[hi])].copy(),
                        'inc_offsets': ioff[lo:hi + 1] - ioff[lo], 'row_vertex': rv[at:at + k].copy(),
                        'event': dict(zip(VERTEX_EVENT, (int(x) for x in ev[i])))})
            at += k
        return res

    def _finish_cluster_vertices(self, sess, vtx, objects, voxels_or_lists, res, spec, shape, value=None):
        """The vertices enqueued with a voxel-score call, or -- the incidence table was too small -- ``cluster_vertices`` on the
        returned ids."""
        got = self._fetch_cluster_vertices(vtx, objects)
        if got is None:
            got = self.cluster_vertices(sess, voxels_or_lists, value() if callable(value) else value, res, spec, shape=shape)
        return got

    def cluster_vertices(self, sess, voxels_or_lists, value, clusters, spec, shape=None):
        """Vertex candidates of clusters already made: ``voxels_or_lists``, ``value``, ``clusters`` and ``shape`` as
        ``cluster_features`` takes them, ``spec`` a ``clusters.ClusterVertexSpec``.  Runs the object records and then the vertices;
        the incidence table starts at 4 K + 1024 entries for K clusters and doubles while the device reports more.  Returns per
        event a dict: ``objects`` (as ``cluster_features``), ``vertices`` (named columns ``clusters.VERTEX_INT`` / ``VERTEX_REAL``,
        one row per vertex), ``incidence`` int64 [I, 5] (``clusters.VERTEX_INCIDENCE``) with ``inc_offsets`` [V_i + 1], event-local:
        the incidences of vertex v are ``inc_offsets[v] .. inc_offsets[v + 1]``, ``row_vertex`` int32 [K_i, 2] and ``event`` (a dict
        over ``clusters.VERTEX_EVENT``).  The record counts ends, bodies and angles; what kind of vertex it is stays the
        consumer's judgement."""
        import torch
        from .clusters import ClusterVertexSpec
        if not isinstance(spec, ClusterVertexSpec):
            raise ValueError('cluster_vertices: spec = %r, expected a clusters.ClusterVertexSpec' % (spec,))
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        if len(shape) not in (2, 3) or any(not 1 <= s <= 32768 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_vertices: shape = %r, expected 2 or 3 extents in [1, 32768] with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, VoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = voxels_or_lists.value
        elif isinstance(voxels_or_lists, _DeviceVoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = self._resident_value(voxels_or_lists)
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_vertices: %d events outside [1, 65535]' % n)
        if isinstance(value, (list, tuple)):
            value = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in value]) if len(value) else np.zeros(0, np.float32)
        if value is not None:
            value = np.asarray(value, np.float32).reshape(-1)
        ids, tables = clusters['cluster'], clusters['clusters']
        if len(ids) != n or len(tables) != n:
            raise ValueError('cluster_vertices: %d events, clusters of %d / %d' % (n, len(ids), len(tables)))
        cluster = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in ids]) if n else np.zeros(0, np.int32)
        if cluster.size != M or index.size != M or (value is not None and value.size != M):
            raise ValueError('cluster_vertices: %d list entries, %d indices, %d ids, %s values'
                             % (M, index.size, cluster.size, 'no' if value is None else value.size))
        toff = np.concatenate([[0], np.cumsum([int(t['first'].size) for t in tables])]).astype(np.int64)
        K = int(toff[-1])
        cls = np.concatenate([np.asarray(t['cls'], np.uint8).reshape(-1) for t in tables] + [np.zeros(1, np.uint8)])
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self._device)
        d_off, d_index, d_toff, d_cls = up(off, np.int64), up(index, np.int32), up(toff, np.int64), up(cls, np.uint8)
        d_cluster = up(cluster if M else np.zeros(1, np.int32), np.int32)
        d_value = None if value is None else up(value if M else np.zeros(1, np.float32), np.float32)
        pending = (d_cluster, None, d_toff, M, n, M)
        dev_objects = self._enqueue_cluster_features(sess, d_off, d_index, d_value, pending, shape)
        objects = self._fetch_cluster_features(dev_objects, tables)
        inc_cap = self._vertex_inc_cap(K)
        while True:
            vtx = self._enqueue_cluster_vertices(sess, d_off, d_index, pending, dev_objects, d_cls, shape, spec, K, inc_cap)
            got = self._fetch_cluster_vertices(vtx, objects)
            if got is not None:
                return got
            if inc_cap >= 2 ** 30 - 1:
                raise _lib.UrsnError('cluster_vertices: more than 2^30 - 1 distinct incidences')
            inc_cap = min(2 * inc_cap, 2 ** 30 - 1)

    # ------------------------------------------------------------------------------------------
    # cluster chains: broken track fragments joined end to end (definition and numpy statement: clusters.cluster_chains_numpy,
    # device passes: csrc/cluster_chain.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_chains(self, spec):
        """A ``clusters.ClusterChainSpec``: while one is set, and a cluster spec is set, and ``'cluster'`` is wanted,
        ``inference_voxel_scores`` and ``inference_tiled_voxel_scores`` enqueue ``ursn_cluster_chains`` behind the cluster passes
        and the object records (which run for it whether or not ``set_cluster_features`` is on; tiled: on the stitched list in the
        large shape, so a track cut at a tile seam with lost voxels is joined), and the result gains ``chains``: what
        ``cluster_chains`` returns.  No table of the call can overflow (there are at most as many chains and joins as clusters),
        so nothing is ever made again.  None switches it off.  The legal members of ``want`` do not change; never called, the
        results have the keys they had."""
        from .clusters import ClusterChainSpec
        if spec is not None and not isinstance(spec, ClusterChainSpec):
            raise ValueError('set_cluster_chains: spec = %r, expected a clusters.ClusterChainSpec or None' % (spec,))
        self._cluster_chain_spec = spec

    def _enqueue_cluster_chains(self, sess, d_offsets, d_index, pending, objects, d_cls, shape, spec, rows):
        """``ursn_cluster_chains`` behind ``_enqueue_cluster_features`` (whose tables stay on the device); ``rows`` bounds the
        cluster rows (the list length when the count is still on the device); enqueues only."""
        import torch
        lib = _lib.load()
        ints, _, toff, _, n, M = pending
        itab, rtab, _ = objects
        shape = [int(s) for s in shape]
        rows = int(rows)
        need = int(lib.ursn_cluster_chains_scratch_bytes(n, M))
        if need == 0:
            raise ValueError('cluster_chains: %d events with %d list entries are out of domain' % (n, M))
        if d_cls is None and (spec.same_class or spec.classes is not None):
            raise ValueError('cluster_chains: spec = %r needs the cluster table\'s cls' % (spec,))
        new = lambda shp, dt: torch.empty(shp, dtype=dt, device=self._device)
        cap = max(rows, 1)
        scratch = new(need // 8, torch.int64)
        merged, small = new(max(M, 1), torch.int32), new(2 * cap, torch.int32)                # small: first | size
        coff, joff, ev, status = new(n + 1, torch.int64), new(n + 1, torch.int64), new((n, _lib.CLCHAIN_EV), torch.int64), \
            new(1, torch.int32)
        ccls = new(cap, torch.uint8)
        ci, cr = new((cap, _lib.CLCHAIN_CI), torch.int64), new((cap, _lib.CLCHAIN_CR), torch.float64)
        ji, jr = new((cap, _lib.CLCHAIN_JI), torch.int64), new((cap, _lib.CLCHAIN_JR), torch.float64)
        rc, rj, rn = new(cap, torch.int32), new((cap, 2), torch.int32), new((cap, 2), torch.int32)
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_chain_desc()
        d.ndim, d.n, d.m_total, d.max_gap = len(shape), n, M, spec.max_gap
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.cluster, d.table_offsets = ptr(d_offsets), ptr(d_index), ints.data_ptr(), toff.data_ptr()
        d.itab, d.rtab, d.feat_cap, d.cls = itab.data_ptr(), rtab.data_ptr(), M, ptr(d_cls)
        d.min_cos, d.min_size, d.class_mask, d.same_class = spec.min_cos, spec.min_size, spec.class_mask(), int(spec.same_class)
        o = _lib.ursn_cluster_chain_out()
        o.merged, o.chain_offsets, o.first, o.size, o.cls = merged.data_ptr(), coff.data_ptr(), small.data_ptr(), \
            small.data_ptr() + 4 * cap, ccls.data_ptr()
        o.chain_itab, o.chain_rtab, o.cap_chains = ci.data_ptr(), cr.data_ptr(), rows
        o.join_offsets, o.join_itab, o.join_rtab, o.cap_joins = joff.data_ptr(), ji.data_ptr(), jr.data_ptr(), rows
        o.row_chain, o.row_join, o.row_candidates, o.cap_rows = rc.data_ptr(), rj.data_ptr(), rn.data_ptr(), rows
        o.event, o.status = ev.data_ptr(), status.data_ptr()
        _lib.check(lib.ursn_cluster_chains(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, merged, small, coff, joff, ev, status, ccls, ci, cr, ji, jr, rc, rj, rn, itab, rtab) + \
                (() if d_cls is None or not hasattr(d_cls, 'record_stream') else (d_cls,)):
            t.record_stream(cur)
        return merged, small, ccls, coff, ci, cr, joff, ji, jr, rc, rj, rn, ev, status, cap, M

    @staticmethod
    def _fetch_cluster_chains(ch, objects, off):
        """The chain tables as ``cluster_chains`` returns them (``objects``: what ``_fetch_cluster_features`` returned for the same
        rows, ``off`` the list offsets)."""
        from .clusters import CHAIN_EVENT, CHAIN_INT, CHAIN_REAL, JOIN_INT, JOIN_REAL
        merged, small, ccls, coff, ci, cr, joff, ji, jr, rc, rj, rn, ev, status, cap, M = ch
        code = int(status.cpu().numpy()[0])
        if code != 0:
            raise _lib.UrsnError('cluster_chains: the ids, table offsets, lists and object records disagree (status %d)' % code)
        counts = [int(o['n'].shape[0]) for o in objects]
        K = int(sum(counts))
        coff, joff, ev = coff.cpu().numpy(), joff.cpu().numpy(), ev.cpu().numpy()
        C, J = int(coff[-1]), int(joff[-1])
        assert coff[0] == 0 and joff[0] == 0 and C <= K <= cap and J <= K, 'cluster_chains: %d chains and %d joins of %d rows' % (C, J, K)
        merged, small, ccls = merged[:M].cpu().numpy(), small.cpu().numpy(), ccls[:C].cpu().numpy()
        ci, cr, ji, jr = ci[:C].cpu().numpy(), cr[:C].cpu().numpy(), ji[:J].cpu().numpy(), jr[:J].cpu().numpy()
        rc, rj, rn = rc[:K].cpu().numpy(), rj[:K].cpu().numpy(), rn[:K].cpu().numpy()
        events, ids, tables, at = [], [], [], 0
        for i, (o, k) in enumerate(zip(objects, counts)):
            lo, hi, jlo, jhi = int(coff[i]), int(coff[i + 1]), int(joff[i]), int(joff[i + 1])
            chains = {name: ci[lo:hi, c].copy() for c, name in enumerate(CHAIN_INT)}
            chains.update({name: cr[lo:hi, c].copy() for c, name in enumerate(CHAIN_REAL)})
            joins = {name: ji[jlo:jhi, c].copy() for c, name in enumerate(JOIN_INT)}
            joins.update({name: jr[jlo:jhi, c].copy() for c, name in enumerate(JOIN_REAL)})
            events.append({'objects': o, 'chains': chains, 'joins': joins, 'row_chain': rc[at:at + k].copy(),
                           'row_join': rj[at:at + k].copy(), 'row_candidates': rn[at:at + k].copy(),
                           'event': dict(zip(CHAIN_EVENT, (int(x) for x in ev[i])))})
            ids.append(merged[off[i]:off[i + 1]].copy())
            tables.append({'first': small[lo:hi].copy(), 'size': small[cap + lo:cap + hi].copy(), 'cls': ccls[lo:hi].copy()})
            at += k
        return {'events': events, 'cluster': ids, 'clusters': tables}

    def cluster_chains(self, sess, voxels_or_lists, value, clusters, spec, shape=None):
        """Chains of clusters already made: ``voxels_or_lists``, ``value``, ``clusters`` and ``shape`` as ``cluster_features`` takes
        them, ``spec`` a ``clusters.ClusterChainSpec``.  Runs the object records and then the chains.  Returns ``{'events': [...],
        'cluster': [...], 'clusters': [...]}``: per event a dict -- ``objects`` (as ``cluster_features``), ``chains`` (named columns
        ``clusters.CHAIN_INT`` / ``CHAIN_REAL``, one row per chain), ``joins`` (``JOIN_INT`` / ``JOIN_REAL``, one row per join,
        ascending ``key_a``), ``row_chain`` int32 [K_i], ``row_join`` / ``row_candidates`` int32 [K_i, 2] and ``event`` (a dict over
        ``clusters.CHAIN_EVENT``) -- and, as ``cluster`` / ``clusters``, the chains as a clustering of the same lists: the merged
        ids int32 [m_i] and the table ``first`` / ``size`` / ``cls``.  The returned dict is itself a legal ``clusters`` argument
        of ``cluster_features``, ``cluster_profiles``, ``match_clusters``, ``cluster_graph`` and ``cluster_vertices``."""
        import torch
        from .clusters import ClusterChainSpec
        if not isinstance(spec, ClusterChainSpec):
            raise ValueError('cluster_chains: spec = %r, expected a clusters.ClusterChainSpec' % (spec,))
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        if len(shape) not in (2, 3) or any(not 1 <= s <= 32768 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_chains: shape = %r, expected 2 or 3 extents in [1, 32768] with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, VoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = voxels_or_lists.value
        elif isinstance(voxels_or_lists, _DeviceVoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = self._resident_value(voxels_or_lists)
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_chains: %d events outside [1, 65535]' % n)
        if isinstance(value, (list, tuple)):
            value = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in value]) if len(value) else np.zeros(0, np.float32)
        if value is not None:
            value = np.asarray(value, np.float32).reshape(-1)
        ids, tables = clusters['cluster'], clusters['clusters']
        if len(ids) != n or len(tables) != n:
            raise ValueError('cluster_chains: %d events, clusters of %d / %d' % (n, len(ids), len(tables)))
        cluster = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in ids]) if n else np.zeros(0, np.int32)
        if cluster.size != M or index.size != M or (value is not None and value.size != M):
            raise ValueError('cluster_chains: %d list entries, %d indices, %d ids, %s values'
                             % (M, index.size, cluster.size, 'no' if value is None else value.size))
        toff = np.concatenate([[0], np.cumsum([int(t['first'].size) for t in tables])]).astype(np.int64)
        K = int(toff[-1])
        cls = np.concatenate([np.asarray(t['cls'], np.uint8).reshape(-1) for t in tables] + [np.zeros(1, np.uint8)])
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self._device)
        d_off, d_index, d_toff, d_cls = up(off, np.int64), up(index, np.int32), up(toff, np.int64), up(cls, np.uint8)
        d_cluster = up(cluster if M else np.zeros(1, np.int32), np.int32)
        d_value = None if value is None else up(value if M else np.zeros(1, np.float32), np.float32)
        pending = (d_cluster, None, d_toff, M, n, M)
        dev_objects = self._enqueue_cluster_features(sess, d_off, d_index, d_value, pending, shape)
        objects = self._fetch_cluster_features(dev_objects, tables)
        ch = self._enqueue_cluster_chains(sess, d_off, d_index, pending, dev_objects, d_cls, shape, spec, K)
        return self._fetch_cluster_chains(ch, objects, off)

    # ------------------------------------------------------------------------------------------
    # cluster cones: shower fragments gathered to their primary (definition and numpy statement: clusters.cluster_cones_numpy,
    # device passes: csrc/cluster_cone.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_cones(self, spec):
        """A ``clusters.ClusterConeSpec``: while one is set, and a cluster spec is set, and ``'cluster'`` is wanted,
        ``inference_voxel_scores`` and ``inference_tiled_voxel_scores`` enqueue ``ursn_cluster_cones`` behind the cluster passes
        and the object records (which run for it whether or not ``set_cluster_features`` is on; tiled: on the stitched list in the
        large shape, so a shower crosses tile seams), and the result gains ``cones``: what ``cluster_cones`` returns.  No table of
        the call can overflow (there are at most as many showers and links as clusters), so nothing is ever made again.  None
        switches it off.  The legal members of ``want`` do not change; never called, the results have the keys they had."""
        from .clusters import ClusterConeSpec
        if spec is not None and not isinstance(spec, ClusterConeSpec):
            raise ValueError('set_cluster_cones: spec = %r, expected a clusters.ClusterConeSpec or None' % (spec,))
        self._cluster_cone_spec = spec

    def _enqueue_cluster_cones(self, sess, d_offsets, d_index, pending, objects, d_cls, shape, spec, rows):
        """``ursn_cluster_cones`` behind ``_enqueue_cluster_features`` (whose tables stay on the device); ``rows`` bounds the
        cluster rows (the list length when the count is still on the device); enqueues only."""
        import torch
        lib = _lib.load()
        ints, _, toff, _, n, M = pending
        itab, rtab, _ = objects
        shape = [int(s) for s in shape]
        rows = int(rows)
        need = int(lib.ursn_cluster_cones_scratch_bytes(n, M))
        if need == 0:
            raise ValueError('cluster_cones: %d events with %d list entries are out of domain' % (n, M))
        if d_cls is None and (spec.same_class or spec.classes is not None):
            raise ValueError('cluster_cones: spec = %r needs the cluster table\'s cls' % (spec,))
        new = lambda shp, dt: torch.empty(shp, dtype=dt, device=self._device)
        cap = max(rows, 1)
        scratch = new(need // 8, torch.int64)
        merged, small = new(max(M, 1), torch.int32), new(2 * cap, torch.int32)                # small: first | size
        soff, loff, ev, status = new(n + 1, torch.int64), new(n + 1, torch.int64), new((n, _lib.CLCONE_EV), torch.int64), \
            new(1, torch.int32)
        scls = new(cap, torch.uint8)
        si, sr = new((cap, _lib.CLCONE_SI), torch.int64), new((cap, _lib.CLCONE_SR), torch.float64)
        li, lr = new((cap, _lib.CLCONE_LI), torch.int64), new((cap, _lib.CLCONE_LR), torch.float64)
        rows5 = new((6, cap), torch.int32)                 # row_shower | row_parent | row_candidates | row_depth | row_children [cap, 2]
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_cone_desc()
        d.ndim, d.n, d.m_total, d.reach = len(shape), n, M, spec.reach
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.cluster, d.table_offsets = ptr(d_offsets), ptr(d_index), ints.data_ptr(), toff.data_ptr()
        d.itab, d.rtab, d.feat_cap, d.cls = itab.data_ptr(), rtab.data_ptr(), M, ptr(d_cls)
        d.min_cos, d.min_size, d.class_mask, d.same_class = spec.min_cos, spec.min_size, spec.class_mask(), int(spec.same_class)
        d.seed_size = spec.seed_size
        o = _lib.ursn_cluster_cone_out()
        o.merged, o.shower_offsets, o.first, o.size, o.cls = merged.data_ptr(), soff.data_ptr(), small.data_ptr(), \
            small.data_ptr() + 4 * cap, scls.data_ptr()
        o.shower_itab, o.shower_rtab, o.cap_showers = si.data_ptr(), sr.data_ptr(), rows
        o.link_offsets, o.link_itab, o.link_rtab, o.cap_links = loff.data_ptr(), li.data_ptr(), lr.data_ptr(), rows
        at = rows5.data_ptr()
        o.row_shower, o.row_parent, o.row_candidates, o.row_depth, o.row_children = at, at + 4 * cap, at + 8 * cap, at + 12 * cap, \
            at + 16 * cap
        o.cap_rows = rows
        o.event, o.status = ev.data_ptr(), status.data_ptr()
        _lib.check(lib.ursn_cluster_cones(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, merged, small, soff, loff, ev, status, scls, si, sr, li, lr, rows5, itab, rtab) + \
                (() if d_cls is None or not hasattr(d_cls, 'record_stream') else (d_cls,)):
            t.record_stream(cur)
        return merged, small, scls, soff, si, sr, loff, li, lr, rows5, ev, status, cap, M

    @staticmethod
    def _fetch_cluster_cones(cn, objects, off):
        """The shower tables as ``cluster_cones`` returns them (``objects``: what ``_fetch_cluster_features`` returned for the same
        rows, ``off`` the list offsets)."""
        from .clusters import CONE_EVENT, CONE_INT, CONE_REAL, LINK_INT, LINK_REAL
        merged, small, scls, soff, si, sr, loff, li, lr, rows5, ev, status, cap, M = cn
        code = int(status.cpu().numpy()[0])
        if code != 0:
            raise _lib.UrsnError('cluster_cones: the ids, table offsets, lists and object records disagree (status %d)' % code)
        counts = [int(o['n'].shape[0]) for o in objects]
        K = int(sum(counts))
        soff, loff, ev = soff.cpu().numpy(), loff.cpu().numpy(), ev.cpu().numpy()
        S, L = int(soff[-1]), int(loff[-1])
        assert soff[0] == 0 and loff[0] == 0 and S <= K <= cap and L <= K, 'cluster_cones: %d showers and %d links of %d rows' % (S, L, K)
        merged, small, scls = merged[:M].cpu().numpy(), small.cpu().numpy(), scls[:S].cpu().numpy()
        si, sr, li, lr = si[:S].cpu().numpy(), sr[:S].cpu().numpy(), li[:L].cpu().numpy(), lr[:L].cpu().numpy()
        rows5 = rows5.cpu().numpy()
        kids = rows5[4:].reshape(cap, 2)
        events, ids, tables, at = [], [], [], 0
        for i, (o, k) in enumerate(zip(objects, counts)):
            lo, hi, llo, lhi = int(soff[i]), int(soff[i + 1]), int(loff[i]), int(loff[i + 1])
            showers = {name: si[lo:hi, c].copy() for c, name in enumerate(CONE_INT)}
            showers.update({name: sr[lo:hi, c].copy() for c, name in enumerate(CONE_REAL)})
            links = {name: li[llo:lhi, c].copy() for c, name in enumerate(LINK_INT)}
            links.update({name: lr[llo:lhi, c].copy() for c, name in enumerate(LINK_REAL)})
            events.append({'objects': o, 'showers': showers, 'links': links, 'row_shower': rows5[0, at:at + k].copy(),
                           'row_parent': rows5[1, at:at + k].copy(), 'row_candidates': rows5[2, at:at + k].copy(),
                           'row_depth': rows5[3, at:at + k].copy(), 'row_children': kids[at:at + k].copy(),
                           'event': dict(zip(CONE_EVENT, (int(x) for x in ev[i])))})
            ids.append(merged[off[i]:off[i + 1]].copy())
            tables.append({'first': small[lo:hi].copy(), 'size': small[cap + lo:cap + hi].copy(), 'cls': scls[lo:hi].copy()})
            at += k
        return {'events': events, 'cluster': ids, 'clusters': tables}

    def cluster_cones(self, sess, voxels_or_lists, value, clusters, spec, shape=None):
        """Showers of clusters already made: ``voxels_or_lists``, ``value``, ``clusters`` and ``shape`` as ``cluster_features`` takes
        them (``clusters`` may be the dict ``cluster_chains`` returned: cones on chains), ``spec`` a ``clusters.ClusterConeSpec``.
        Runs the object records and then the cones.  Returns ``{'events': [...], 'cluster': [...], 'clusters': [...]}``: per event a
        dict -- ``objects`` (as ``cluster_features``), ``showers`` (named columns ``clusters.CONE_INT`` / ``CONE_REAL``, one row per
        shower), ``links`` (``LINK_INT`` / ``LINK_REAL``, one row per link, ascending child row), ``row_shower`` / ``row_parent`` /
        ``row_candidates`` / ``row_depth`` int32 [K_i], ``row_children`` int32 [K_i, 2] and ``event`` (a dict over
        ``clusters.CONE_EVENT``) -- and, as ``cluster`` / ``clusters``, the showers as a clustering of the same lists: the merged
        ids int32 [m_i] and the table ``first`` / ``size`` / ``cls``.  The returned dict is itself a legal ``clusters`` argument
        of the other cluster calls."""
        import torch
        from .clusters import ClusterConeSpec
        if not isinstance(spec, ClusterConeSpec):
            raise ValueError('cluster_cones: spec = %r, expected a clusters.ClusterConeSpec' % (spec,))
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        if len(shape) not in (2, 3) or any(not 1 <= s <= 32768 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_cones: shape = %r, expected 2 or 3 extents in [1, 32768] with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, VoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = voxels_or_lists.value
        elif isinstance(voxels_or_lists, _DeviceVoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = self._resident_value(voxels_or_lists)
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_cones: %d events outside [1, 65535]' % n)
        if isinstance(value, (list, tuple)):
            value = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in value]) if len(value) else np.zeros(0, np.float32)
        if value is not None:
            value = np.asarray(value, np.float32).reshape(-1)
        ids, tables = clusters['cluster'], clusters['clusters']
        if len(ids) != n or len(tables) != n:
            raise ValueError('cluster_cones: %d events, clusters of %d / %d' % (n, len(ids), len(tables)))
        cluster = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in ids]) if n else np.zeros(0, np.int32)
        if cluster.size != M or index.size != M or (value is not None and value.size != M):
            raise ValueError('cluster_cones: %d list entries, %d indices, %d ids, %s values'
                             % (M, index.size, cluster.size, 'no' if value is None else value.size))
        toff = np.concatenate([[0], np.cumsum([int(t['first'].size) for t in tables])]).astype(np.int64)
        K = int(toff[-1])
        cls = np.concatenate([np.asarray(t['cls'], np.uint8).reshape(-1) for t in tables] + [np.zeros(1, np.uint8)])
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self._device)
        d_off, d_index, d_toff, d_cls = up(off, np.int64), up(index, np.int32), up(toff, np.int64), up(cls, np.uint8)
        d_cluster = up(cluster if M else np.zeros(1, np.int32), np.int32)
        d_value = None if value is None else up(value if M else np.zeros(1, np.float32), np.float32)
        pending = (d_cluster, None, d_toff, M, n, M)
        dev_objects = self._enqueue_cluster_features(sess, d_off, d_index, d_value, pending, shape)
        objects = self._fetch_cluster_features(dev_objects, tables)
        cn = self._enqueue_cluster_cones(sess, d_off, d_index, pending, dev_objects, d_cls, shape, spec, K)
        return self._fetch_cluster_cones(cn, objects, off)

    # ------------------------------------------------------------------------------------------
    # cluster matching (definition and numpy statement: clusters.cluster_match_numpy, device passes: csrc/cluster_match.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_matching(self, on):
        """While on, and a cluster spec is set, and ``'cluster'`` is wanted, ``inference_voxel_scores`` (``with_labels``) and
        ``inference_tiled_voxel_scores`` also cluster the TRUE classes -- the batch's resident label list cast to uint8 -- under the
        same spec and enqueue ``ursn_cluster_match`` behind it with the resident value list; the result gains ``true_cluster`` /
        ``true_clusters`` (as ``cluster`` / ``clusters``) and ``match`` (as ``match_clusters`` returns it, A = predicted, B = true).
        A batch without labels is then refused.  The legal members of ``want`` do not change; never called, the results have the
        keys they had."""
        if type(on) is not bool:
            raise ValueError('set_cluster_matching: on = %r, expected a bool' % (on,))
        self._cluster_matching_on = on

    @staticmethod
    def _label_classes(label, M):
        """The float label list on the device as the uint8 classes ``ursn_cluster_voxels`` reads (a cast: plumbing)."""
        import torch
        if M == 0:
            return torch.zeros(1, dtype=torch.uint8, device=label.device)
        return label[:M].clamp(0, 255).to(torch.uint8)

    def _enqueue_cluster_match(self, sess, d_offsets, side_a, side_b, d_value, n, M, pairs):
        """``ursn_cluster_match`` behind two ``_enqueue_clusters`` (``side_a`` / ``side_b``: what they returned; the ids and table
        offsets stay on the device); enqueues only."""
        import torch
        lib = _lib.load()
        cap = M
        need = int(lib.ursn_cluster_match_scratch_bytes(n, M, cap, cap, cap))
        if need == 0:
            raise ValueError('match_clusters: %d events with %d list entries are out of domain' % (n, M))
        scratch = torch.empty(need // 8, dtype=torch.int64, device=self._device)
        I, R, EI, ER = _lib.CLMATCH_I, _lib.CLMATCH_R, _lib.CLMATCH_EI, _lib.CLMATCH_ER
        rows = max(cap, 1)
        ints = torch.empty(2 * rows * I + n * EI + (rows + 1) + 2 * rows, dtype=torch.int64, device=self._device)
        reals = torch.empty(2 * rows * R + n * ER, dtype=torch.float64, device=self._device)
        small = torch.empty(rows + 1, dtype=torch.int32, device=self._device)     # pair_b | status
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_match_desc()
        d.n, d.m_total, d.offsets, d.value = n, M, ptr(d_offsets), ptr(d_value)
        d.cluster_a, d.table_offsets_a = side_a[0].data_ptr(), side_a[2].data_ptr()
        d.cluster_b, d.table_offsets_b = side_b[0].data_ptr(), side_b[2].data_ptr()
        o = _lib.ursn_cluster_match_out()
        ib, rb = ints.data_ptr(), reals.data_ptr()
        o.a_int, o.b_int, o.event_int = ib, ib + 8 * rows * I, ib + 16 * rows * I
        o.a_real, o.b_real, o.event_real = rb, rb + 8 * rows * R, rb + 16 * rows * R
        o.cap_a = o.cap_b = cap
        at = 16 * rows * I + 8 * n * EI
        if pairs:
            o.pair_offsets, o.pair_n, o.pair_q = ib + at, ib + at + 8 * (rows + 1), ib + at + 8 * (rows + 1) + 8 * rows
            o.pair_b, o.pair_cap = small.data_ptr(), cap
        o.status = small.data_ptr() + 4 * rows
        _lib.check(lib.ursn_cluster_match(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, ints, reals, small):
            t.record_stream(cur)
        return ints, reals, small, rows, n, pairs

    @staticmethod
    def _fetch_cluster_match(pending, tables_a, tables_b):
        """The records as per-event dicts of named arrays for either side, named arrays for the events and, with ``pairs``, per
        event ``(a, b, n, q)``; raises on a non-zero status."""
        from .clusters import MATCH_EVENT_INT, MATCH_EVENT_REAL, MATCH_ROW_INT, MATCH_ROW_REAL
        ints, reals, small, rows, n, pairs = pending
        I, R, EI, ER = _lib.CLMATCH_I, _lib.CLMATCH_R, _lib.CLMATCH_EI, _lib.CLMATCH_ER
        code = int(small[rows:].cpu().numpy()[0])
        if code != 0:
            raise _lib.UrsnError('match_clusters: the ids, table offsets and lists disagree (status %d)' % code)
        counts = [[int(t['first'].size) for t in tables] for tables in (tables_a, tables_b)]
        total = [int(sum(c)) for c in counts]
        assert max(total) <= rows, 'match_clusters: %r rows, room for %d' % (total, rows)
        hi, hr = ints.cpu().numpy(), reals.cpu().numpy()
        res = {}
        for x, side in enumerate('ab'):
            it = hi[x * rows * I:(x * rows + total[x]) * I].reshape(total[x], I)
            rt = hr[x * rows * R:(x * rows + total[x]) * R].reshape(total[x], R)
            per, at = [], 0
            for k in counts[x]:
                ev = {name: it[at:at + k, c].copy() for c, name in enumerate(MATCH_ROW_INT)}
                ev.update({name: rt[at:at + k, c].copy() for c, name in enumerate(MATCH_ROW_REAL)})
                per.append(ev)
                at += k
            res[side] = per
        ei = hi[2 * rows * I:2 * rows * I + n * EI].reshape(n, EI)
        er = hr[2 * rows * R:2 * rows * R + n * ER].reshape(n, ER)
        res['events'] = {name: ei[:, c].copy() for c, name in enumerate(MATCH_EVENT_INT)}
        res['events'].update({name: er[:, c].copy() for c, name in enumerate(MATCH_EVENT_REAL)})
        assert np.array_equal(res['events']['rows_a'], counts[0]) and np.array_equal(res['events']['rows_b'], counts[1]), \
            'match_clusters: row counts and the cluster tables disagree'
        if pairs:
            at = 2 * rows * I + n * EI
            po = hi[at:at + total[0] + 1]
            pn, pq = hi[at + rows + 1:at + 2 * rows + 1], hi[at + 2 * rows + 1:at + 3 * rows + 1]
            pb = small[:rows].cpu().numpy()
            assert po[0] == 0 and po[-1] <= rows, 'match_clusters: %d cells, room for %d' % (int(po[-1]), rows)
            res['pairs'], r0 = [], 0
            for k in counts[0]:
                lo, hi_ = int(po[r0]), int(po[r0 + k])
                a = np.repeat(np.arange(k, dtype=np.int32), np.diff(po[r0:r0 + k + 1]))
                res['pairs'].append((a, pb[lo:hi_].copy(), pn[lo:hi_].copy(), pq[lo:hi_].copy()))
                r0 += k
        return res

    def match_clusters(self, sess, voxels_or_lists, clusters_a, clusters_b, value=None, pairs=False):
        """The match of two clusterings of the same lists: ``voxels_or_lists`` as ``cluster_voxels`` took it, ``clusters_a``
        (predicted) and ``clusters_b`` (true) the dicts ``cluster_voxels`` returned (or a result's ``cluster`` / ``clusters`` under
        those keys), ``value`` the entries' values as one flat array or per-event arrays (None: a VoxelBatch's own, or no charge for
        plain lists).  Returns ``{'a': [...], 'b': [...], 'events': {...}}``: per event a dict of arrays with one row per cluster of
        that side (``clusters.MATCH_ROW_INT`` + ``MATCH_ROW_REAL``), named arrays with one row per event (``MATCH_EVENT_INT`` +
        ``MATCH_EVENT_REAL``) and, with ``pairs``, ``pairs``: per event the cells as ``(a, b, n, q)`` arrays, by A id, then B id."""
        import torch
        if isinstance(voxels_or_lists, VoxelBatch):
            off = np.asarray(voxels_or_lists.offsets, np.int64)
            if value is None:
                value = voxels_or_lists.value
        else:
            sizes = [np.asarray(a).size for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('match_clusters: %d events outside [1, 65535]' % n)
        if type(pairs) is not bool:
            raise ValueError('match_clusters: pairs = %r, expected a bool' % (pairs,))
        if isinstance(value, (list, tuple)):
            value = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in value]) if len(value) else np.zeros(0, np.float32)
        if value is not None:
            value = np.asarray(value, np.float32).reshape(-1)
            if value.size != M:
                raise ValueError('match_clusters: %d list entries, %d values' % (M, value.size))
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self._device)
        sides = []
        for name, c in (('clusters_a', clusters_a), ('clusters_b', clusters_b)):
            ids, tables = c['cluster'], c['clusters']
            if len(ids) != n or len(tables) != n:
                raise ValueError('match_clusters: %d events, %s of %d / %d' % (n, name, len(ids), len(tables)))
            flat = np.concatenate([np.asarray(i, np.int32).reshape(-1) for i in ids])
            if flat.size != M or any(np.asarray(i).size != off[e + 1] - off[e] for e, i in enumerate(ids)):
                raise ValueError('match_clusters: the ids of %s do not have the lengths of the lists' % name)
            toff = np.concatenate([[0], np.cumsum([int(t['first'].size) for t in tables])]).astype(np.int64)
            sides.append((up(flat if M else np.zeros(1, np.int32), np.int32), None, up(toff, np.int64)))
        d_value = None if value is None else up(value if M else np.zeros(1, np.float32), np.float32)
        pending = self._enqueue_cluster_match(sess, up(off, np.int64), sides[0], sides[1], d_value, n, M, pairs)
        return self._fetch_cluster_match(pending, clusters_a['clusters'], clusters_b['clusters'])

    # ------------------------------------------------------------------------------------------
    # cluster contact graph (definition and numpy statement: clusters.cluster_graph_numpy, device passes: csrc/cluster_graph.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_graph(self, spec):
        """A ``clusters.ClusterGraphSpec``, while a cluster spec is set and ``'cluster'`` is wanted, makes
        ``inference_voxel_scores`` and ``inference_tiled_voxel_scores`` enqueue ``ursn_cluster_graph`` behind the cluster passes
        (tiled: on the stitched list in the large shape, so groups cross tile borders), with the batch's own resident value list;
        the result gains ``graph`` (as ``cluster_graph`` returns it).  None takes it away again.  The legal members of ``want`` do
        not change; never called, the results have the keys they had."""
        from .clusters import ClusterGraphSpec
        if spec is not None and not isinstance(spec, ClusterGraphSpec):
            raise ValueError('set_cluster_graph: spec = %r, expected a clusters.ClusterGraphSpec or None' % (spec,))
        self._cluster_graph_spec = spec

    def _enqueue_cluster_graph(self, sess, d_offsets, d_index, d_value, d_cluster, d_toff, d_cls, n, M, shape, spec, edge_cap, edges):
        """``ursn_cluster_graph`` on device lists, ids and table offsets (raw pointers or tensors); enqueues only."""
        import torch
        lib = _lib.load()
        shape = [int(s) for s in shape]
        edge_cap = int(min(max(edge_cap, 0), 2 ** 30 - 1))
        cap = M
        need = int(lib.ursn_cluster_graph_scratch_bytes(n, M, cap, cap, edge_cap))
        if need == 0:
            raise ValueError('cluster_graph: %d events with %d list entries are out of domain' % (n, M))
        E, I, G, EV = _lib.CLGRAPH_E, _lib.CLGRAPH_I, _lib.CLGRAPH_G, _lib.CLGRAPH_EV
        rows, ecap = max(cap, 1), max(edge_cap, 1)
        scratch = torch.empty(need // 8, dtype=torch.int64, device=self._device)
        # rows | groups | group_offsets | event | edge_offsets | edges
        ints = torch.empty(rows * (I + G) + (n + 1) + n * EV + (rows + 1) + (ecap * E if edges else 0), dtype=torch.int64,
                           device=self._device)
        small = torch.empty(rows + 1, dtype=torch.int32, device=self._device)      # group | status
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_graph_desc()
        d.ndim, d.n, d.gap, d.m_total, d.edge_cap = len(shape), n, spec.gap, M, edge_cap
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.cluster, d.table_offsets = ptr(d_offsets), ptr(d_index), ptr(d_cluster), ptr(d_toff)
        d.value, d.cls = ptr(d_value), ptr(d_cls)
        o = _lib.ursn_cluster_graph_out()
        at = ints.data_ptr()
        o.rows, o.cap_rows = at, cap
        o.groups, o.cap_groups = at + 8 * rows * I, cap
        o.group_offsets = at + 8 * rows * (I + G)
        o.event = o.group_offsets + 8 * (n + 1)
        if edges:
            o.edge_offsets = o.event + 8 * n * EV
            o.edges, o.edge_out_cap = o.edge_offsets + 8 * (rows + 1), edge_cap
        o.group, o.status = small.data_ptr(), small.data_ptr() + 4 * rows
        _lib.check(lib.ursn_cluster_graph(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, ints, small):
            t.record_stream(cur)
        return ints, small, rows, ecap, n, M, edges

    @staticmethod
    def _fetch_cluster_graph(pending, off, counts):
        """The tables as per-event dicts (``counts``: rows per event), or None when the edge table was too small; raises on any
        other status."""
        from .clusters import GRAPH_EDGE, GRAPH_EVENT, GRAPH_GROUP, GRAPH_ROW
        ints, small, rows, ecap, n, M, edges = pending
        E, I, G, EV = _lib.CLGRAPH_E, _lib.CLGRAPH_I, _lib.CLGRAPH_G, _lib.CLGRAPH_EV
        hs = small.cpu().numpy()
        code = int(hs[rows])
        if code == _lib.CLGRAPH_EDGE_OVERFLOW:
            return None
        if code != 0:
            raise _lib.UrsnError('cluster_graph: the ids, table offsets and lists disagree (status %d)' % code)
        total = int(sum(counts))
        assert total <= rows, 'cluster_graph: %d rows, room for %d' % (total, rows)
        hi = ints.cpu().numpy()
        rt = hi[:total * I].reshape(total, I)
        goff = hi[rows * (I + G):rows * (I + G) + n + 1]
        gt = hi[rows * I:rows * I + int(goff[-1]) * G].reshape(int(goff[-1]), G)
        at = rows * (I + G) + n + 1
        ev = hi[at:at + n * EV].reshape(n, EV)
        at += n * EV
        res, r0 = [], 0
        if edges:
            eoff = hi[at:at + total + 1]
            et = hi[at + rows + 1:at + rows + 1 + int(eoff[-1]) * E].reshape(int(eoff[-1]), E)
        for i, k in enumerate(counts):
            one = {'rows': {name: rt[r0:r0 + k, c].copy() for c, name in enumerate(GRAPH_ROW)},
                   'groups': {name: gt[goff[i]:goff[i + 1], c].copy() for c, name in enumerate(GRAPH_GROUP)},
                   'group': hs[off[i]:off[i + 1]].copy(),
                   'event': {name: int(ev[i, c]) for c, name in enumerate(GRAPH_EVENT)}}
            if edges:
                lo = int(eoff[r0])
                one['edge_offsets'] = (eoff[r0:r0 + k + 1] - lo).copy()
                one['edges'] = {name: et[lo:int(eoff[r0 + k]), c].copy() for c, name in enumerate(GRAPH_EDGE)}
            res.append(one)
            r0 += k
        return res

    def _finish_cluster_graph(self, sess, pending, voxels_or_lists, res, spec, shape, value=None):
        """The graph enqueued with a voxel-score call, or -- its edge table was too small -- ``cluster_graph`` on the returned ids."""
        counts = [int(t['first'].size) for t in res['clusters']]
        off = np.concatenate([[0], np.cumsum([np.asarray(c).size for c in res['cluster']])]).astype(np.int64)
        got = self._fetch_cluster_graph(pending, off, counts)
        if got is None:
            got = self.cluster_graph(sess, voxels_or_lists, res, spec, value=value() if callable(value) else value, shape=shape)
        return got

    @staticmethod
    def _resident_value(batch):
        """The value list of an uploaded batch, read back from the device."""
        import torch
        if batch.m == 0:
            return np.zeros(0, np.float32)
        at = batch.ptr['value'] - batch.dev.data_ptr()
        return batch.dev[at:at + 4 * batch.m].view(torch.float32).cpu().numpy()

    def cluster_graph(self, sess, voxels_or_lists, clusters, spec, value=None, shape=None, edges=True):
        """The contact graph and interaction groups of clusters already made: ``voxels_or_lists`` and ``shape`` as
        ``cluster_voxels`` took them, ``clusters`` the dict it returned (or a result's ``cluster`` / ``clusters`` under those keys),
        ``spec`` a ``clusters.ClusterGraphSpec``, ``value`` the entries' values as one flat array or per-event arrays (None: a
        VoxelBatch's own, or no charge for plain lists).  Returns per event a dict: ``rows`` (columns ``clusters.GRAPH_ROW``, one
        row per cluster), ``groups`` (columns ``GRAPH_GROUP``), ``group`` (int32 [m_i]), ``event`` (``GRAPH_EVENT`` as integers)
        and, with ``edges``, ``edge_offsets`` [K_i + 1] and ``edges`` (columns ``GRAPH_EDGE``; ``pos_a`` / ``pos_b`` are positions
        in the concatenated list).  The edge table starts at ``4 K_total + 1024`` edges and doubles while the device reports that it
        was too small, up to the number of row pairs."""
        import torch
        from .clusters import ClusterGraphSpec
        if not isinstance(spec, ClusterGraphSpec):
            raise ValueError('cluster_graph: spec = %r, expected a clusters.ClusterGraphSpec' % (spec,))
        if type(edges) is not bool:
            raise ValueError('cluster_graph: edges = %r, expected a bool' % (edges,))
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        if len(shape) not in (2, 3) or any(not 1 <= s <= 32768 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_graph: shape = %r, expected 2 or 3 extents in [1, 32768] with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, VoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = voxels_or_lists.value
        elif isinstance(voxels_or_lists, _DeviceVoxelBatch):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
            if value is None:
                value = self._resident_value(voxels_or_lists)
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_graph: %d events outside [1, 65535]' % n)
        if isinstance(value, (list, tuple)):
            value = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in value]) if len(value) else np.zeros(0, np.float32)
        if value is not None:
            value = np.asarray(value, np.float32).reshape(-1)
        ids, tables = clusters['cluster'], clusters['clusters']
        if len(ids) != n or len(tables) != n:
            raise ValueError('cluster_graph: %d events, clusters of %d / %d' % (n, len(ids), len(tables)))
        cluster = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in ids])
        if cluster.size != M or index.size != M or (value is not None and value.size != M):
            raise ValueError('cluster_graph: %d list entries, %d indices, %d ids, %s values'
                             % (M, index.size, cluster.size, 'no' if value is None else value.size))
        counts = [int(t['first'].size) for t in tables]
        toff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        cls = np.concatenate([np.asarray(t['cls'], np.uint8).reshape(-1) for t in tables])
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, dt), dtype=dt)).to(self._device)
        d_off, d_index, d_toff, d_cluster, d_cls = up(off, np.int64), up(index, np.int32), up(toff, np.int64), \
            up(cluster, np.int32), up(cls, np.uint8)
        d_value = None if value is None else up(value, np.float32)
        most = sum(k * (k - 1) // 2 for k in counts)          # no more edges than pairs of rows
        edge_cap = 4 * int(toff[-1]) + 1024
        while True:
            pending = self._enqueue_cluster_graph(sess, d_off, d_index, d_value, d_cluster, d_toff, d_cls, n, M, shape, spec,
                                                  edge_cap, edges)
            got = self._fetch_cluster_graph(pending, off, counts)
            if got is not None:
                return got
            if edge_cap >= most or edge_cap >= 2 ** 30 - 1:
                raise _lib.UrsnError('cluster_graph: the edge table overflowed at %d edges, the number of row pairs' % edge_cap)
            edge_cap = min(2 * edge_cap, max(most, 1), 2 ** 30 - 1)

    # ------------------------------------------------------------------------------------------
    # cluster splits: a component of several particles cut at its junctions and kinks (definition and numpy statement:
    # clusters.cluster_split_numpy, device passes: csrc/cluster_split.hip)
    # ------------------------------------------------------------------------------------------
    def set_cluster_split(self, spec, downstream=False):
        """A ``clusters.ClusterSplitSpec``: while one is set, and a cluster spec is set, and ``'cluster'`` is wanted,
        ``inference_voxel_scores`` and ``inference_tiled_voxel_scores`` enqueue ``ursn_cluster_split`` behind the cluster passes
        (tiled: on the stitched list in the large shape) and the result gains ``split``: what ``cluster_split`` returns.  With
        ``downstream`` the object records, profiles, vertices, chains, cones and graph of those calls run on the pieces instead of
        the components; ``cluster`` / ``clusters`` and matching stay on the components.  None switches it off; never called, the
        results are what they were."""
        from .clusters import ClusterSplitSpec
        if spec is not None and not isinstance(spec, ClusterSplitSpec):
            raise ValueError('set_cluster_split: spec = %r, expected a clusters.ClusterSplitSpec or None' % (spec,))
        if type(downstream) is not bool:
            raise ValueError('set_cluster_split: downstream = %r, expected a bool' % (downstream,))
        self._cluster_split_spec, self._cluster_split_downstream = spec, bool(downstream and spec is not None)

    def _enqueue_cluster_split(self, sess, d_offsets, d_index, d_cluster, d_toff, d_size, d_cls, n, M, shape, spec, cap_pieces,
                               cap_junctions, cap_rows):
        """``ursn_cluster_split`` on device lists, ids, table offsets and the table's size / cls (raw pointers or tensors); enqueues
        only.  The piece table it writes stays on the device for the calls that run on the pieces."""
        import torch
        lib = _lib.load()
        shape = [int(s) for s in shape]
        need = int(lib.ursn_cluster_split_scratch_bytes(n, M))
        if need == 0:
            raise ValueError('cluster_split: %d events with %d list entries are out of domain' % (n, M))
        if d_cls is None and spec.classes is not None:
            raise ValueError('cluster_split: spec = %r needs the cluster table\'s cls' % (spec,))
        new = lambda shp, dt: torch.empty(shp, dtype=dt, device=self._device)
        cp, cj, cr = (int(min(max(c, 0), max(M, 0))) for c in (cap_pieces, cap_junctions, cap_rows))
        scratch = new(need // 8, torch.int64)
        split, mark, small = new(max(M, 1), torch.int32), new(max(M, 1), torch.uint8), new(2 * max(cp, 1), torch.int32)   # first | size
        pcls, pi = new(max(cp, 1), torch.uint8), new((max(cp, 1), _lib.CLSPLIT_PI), torch.int64)
        ji, jr = new((max(cj, 1), _lib.CLSPLIT_JI), torch.int64), new((max(cj, 1), _lib.CLSPLIT_JR), torch.float64)
        rows = new((max(cr, 1), _lib.CLSPLIT_ROW), torch.int32)
        poff, joff, ev, status = new(n + 1, torch.int64), new(n + 1, torch.int64), new((n, _lib.CLSPLIT_EV), torch.int64), \
            new(1, torch.int32)
        ptr = lambda x: None if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else int(x)
        d = _lib.ursn_cluster_split_desc()
        d.ndim, d.n, d.m_total, d.radius = len(shape), n, M, spec.radius
        for i, s in enumerate(shape):
            d.spatial[i] = s
        d.offsets, d.index, d.cluster, d.table_offsets = ptr(d_offsets), ptr(d_index), ptr(d_cluster), ptr(d_toff)
        d.size, d.cls = ptr(d_size), ptr(d_cls)
        d.kink_cos, d.min_size, d.class_mask, d.grow = spec.kink_cos, spec.min_size, spec.class_mask(), spec.grow
        o = _lib.ursn_cluster_split_out()
        o.split, o.mark, o.piece_offsets = split.data_ptr(), mark.data_ptr(), poff.data_ptr()
        o.first, o.size, o.cls = small.data_ptr(), small.data_ptr() + 4 * max(cp, 1), pcls.data_ptr()
        o.piece_itab, o.cap_pieces = pi.data_ptr(), cp
        o.junction_offsets, o.junction_itab, o.junction_rtab, o.cap_junctions = joff.data_ptr(), ji.data_ptr(), jr.data_ptr(), cj
        o.rows, o.cap_rows, o.event, o.status = rows.data_ptr(), cr, ev.data_ptr(), status.data_ptr()
        _lib.check(lib.ursn_cluster_split(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), need, self._stream(sess)))
        cur = torch.cuda.current_stream(self._device)
        for t in (scratch, split, mark, small, pcls, pi, ji, jr, rows, poff, joff, ev, status) + \
                tuple(x for x in (d_cluster, d_toff, d_size, d_cls) if hasattr(x, 'record_stream')):
            t.record_stream(cur)
        return split, mark, small, pcls, pi, ji, jr, rows, poff, joff, ev, status, cp, cj, cr, n, M

    @staticmethod
    def _fetch_cluster_split(sp, off, counts):
        """The tables as ``cluster_split`` returns them (``counts``: cluster rows per event), or the true (pieces, junctions) when a
        table was too small; raises on a status."""
        from .clusters import SPLIT_EVENT, SPLIT_JUNCTION_INT, SPLIT_JUNCTION_REAL, SPLIT_PIECE, SPLIT_ROW
        split, mark, small, pcls, pi, ji, jr, rows, poff, joff, ev, status, cp, cj, cr, n, M = sp
        code = int(status.cpu().numpy()[0])
        if code != 0:
            raise _lib.UrsnError('cluster_split: the ids, table offsets and lists disagree (status %d)' % code)
        poff, joff, ev = poff.cpu().numpy(), joff.cpu().numpy(), ev.cpu().numpy()
        P, J, K = int(poff[-1]), int(joff[-1]), int(sum(counts))
        if P > cp or J > cj:
            return P, J
        assert K <= cr or K == 0, 'cluster_split: %d rows, room for %d' % (K, cr)
        split, mark, small, pcls = split[:M].cpu().numpy(), mark[:M].cpu().numpy(), small.cpu().numpy(), pcls[:P].cpu().numpy()
        pi, ji, jr, rows = pi[:P].cpu().numpy(), ji[:J].cpu().numpy(), jr[:J].cpu().numpy(), rows[:K].cpu().numpy()
        events, ids, tables, at, width = [], [], [], 0, max(cp, 1)
        for i, k in enumerate(counts):
            lo, hi, jlo, jhi = int(poff[i]), int(poff[i + 1]), int(joff[i]), int(joff[i + 1])
            junctions = {name: ji[jlo:jhi, c].copy() for c, name in enumerate(SPLIT_JUNCTION_INT)}
            junctions.update({name: jr[jlo:jhi, c].copy() for c, name in enumerate(SPLIT_JUNCTION_REAL)})
            events.append({'pieces': {name: pi[lo:hi, c].copy() for c, name in enumerate(SPLIT_PIECE)}, 'junctions': junctions,
                           'rows': {name: rows[at:at + k, c].copy() for c, name in enumerate(SPLIT_ROW)},
                           'mark': mark[off[i]:off[i + 1]].copy(), 'event': dict(zip(SPLIT_EVENT, (int(x) for x in ev[i])))})
            ids.append(split[off[i]:off[i + 1]].copy())
            tables.append({'first': small[lo:hi].copy(), 'size': small[width + lo:width + hi].copy(), 'cls': pcls[lo:hi].copy()})
            at += k
        return {'events': events, 'cluster': ids, 'clusters': tables}

    def cluster_split(self, sess, voxels_or_lists, clusters, spec, shape=None):
        """The split of clusters already made: ``voxels_or_lists`` and ``shape`` as ``cluster_voxels`` took them, ``clusters`` the
        dict it returned (or a result's ``cluster`` / ``clusters`` under those keys), ``spec`` a ``clusters.ClusterSplitSpec``.
        Returns ``{'events': [...], 'cluster': [...], 'clusters': [...]}``: per event a dict -- ``pieces`` (named columns
        ``clusters.SPLIT_PIECE``, one row per piece), ``junctions`` (``SPLIT_JUNCTION_INT`` / ``SPLIT_JUNCTION_REAL``, one row per
        junction), ``rows`` (``SPLIT_ROW``, one row per cluster), ``mark`` uint8 [m_i] and ``event`` (a dict over ``SPLIT_EVENT``)
        -- and, as ``cluster`` / ``clusters``, the pieces as a clustering of the same lists: the piece ids int32 [m_i] and the table
        ``first`` / ``size`` / ``cls``.  The returned dict is itself a legal ``clusters`` argument of every call that takes one
        (none of them needs ``first`` to ascend).  The piece and junction tables start at an estimate (4 K + 1024 and K + 1024
        rows); when the device counts more, the call runs once more with the true counts."""
        import torch
        from .clusters import ClusterSplitSpec
        if not isinstance(spec, ClusterSplitSpec):
            raise ValueError('cluster_split: spec = %r, expected a clusters.ClusterSplitSpec' % (spec,))
        shape = [int(s) for s in (self._dims[:-1] if shape is None else shape)]
        if len(shape) not in (2, 3) or any(not 1 <= s <= 32768 for s in shape) or int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
            raise ValueError('cluster_split: shape = %r, expected 2 or 3 extents in [1, 32768] with a product below 2^31' % (shape,))
        if isinstance(voxels_or_lists, (VoxelBatch, _DeviceVoxelBatch)):
            off, index = np.asarray(voxels_or_lists.offsets, np.int64), np.asarray(voxels_or_lists.index, np.int32)
        else:
            lists = [np.asarray(a, np.int32).reshape(-1) for a in voxels_or_lists]
            off = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
            index = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        n, M = off.size - 1, int(off[-1])
        if not 1 <= n <= 65535:
            raise ValueError('cluster_split: %d events outside [1, 65535]' % n)
        ids, tables = clusters['cluster'], clusters['clusters']
        if len(ids) != n or len(tables) != n:
            raise ValueError('cluster_split: %d events, clusters of %d / %d' % (n, len(ids), len(tables)))
        cluster = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c in ids])
        if cluster.size != M or index.size != M:
            raise ValueError('cluster_split: %d list entries, %d indices, %d ids' % (M, index.size, cluster.size))
        counts = [int(t['first'].size) for t in tables]
        toff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        K = int(toff[-1])
        cls = np.concatenate([np.asarray(t['cls'], np.uint8).reshape(-1) for t in tables])
        size = np.concatenate([np.asarray(t['size'], np.int32).reshape(-1) for t in tables])
        if cls.size != K or size.size != K:
            raise ValueError('cluster_split: %d rows, %d sizes, %d classes' % (K, size.size, cls.size))
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, dt), dtype=dt)).to(self._device)
        d_off, d_index, d_toff, d_cluster = up(off, np.int64), up(index, np.int32), up(toff, np.int64), up(cluster, np.int32)
        d_size, d_cls = up(size, np.int32), up(cls, np.uint8)
        est = getattr(self, '_cluster_split_estimate', (4, 1024, 1, 1024))
        cap_pieces, cap_junctions = est[0] * K + est[1], est[2] * K + est[3]
        for _ in range(2):
            sp = self._enqueue_cluster_split(sess, d_off, d_index, d_cluster, d_toff, d_size, d_cls, n, M, shape, spec, cap_pieces,
                                             cap_junctions, K)
            got = self._fetch_cluster_split(sp, off, counts)
            if isinstance(got, dict):
                return got
            cap_pieces, cap_junctions = got
        raise _lib.UrsnError('cluster_split: %d pieces and %d junctions did not fit the tables made for them' % got)

    # ------------------------------------------------------------------------------------------
    # tiling: volumes larger than the network (not in the reference, whose events have the network's size; boxes, their
    # cores and the numpy statement of the device passes: tiling.py)
    # ------------------------------------------------------------------------------------------
    def upload_voxels(self, vb, big):
        """A device-resident LARGE batch: ``vb`` is a VoxelBatch whose events have the shape ``big`` (same number of axes as the
        network, any extents with ``prod(big) < 2^31``), not the network's.  Every array is packed into one page-locked buffer
        and travels in ONE copy on the copy stream, under the staging discipline of ``_feed_voxels``: the call returns once the
        copy is done and never waits for compute.  Unlike a fed batch the device buffer belongs to the returned object and is
        never reused: ``inference_tiled_voxel_scores`` and ``crop=`` read it as often as they like."""
        import torch
        self._require_single_channel('upload_voxels')
        big = tuple(int(s) for s in big)
        if len(big) != len(self._dims) - 1:
            raise ValueError('upload_voxels: big = %r for a network of %d spatial axes' % (big, len(self._dims) - 1))
        if vb.voxels != int(np.prod(big, dtype=np.int64)):
            raise ValueError('upload_voxels: VoxelBatch of %d voxels per event, prod(big) = %d'
                             % (vb.voxels, int(np.prod(big, dtype=np.int64))))
        vb.validate()
        if not 1 <= vb.n <= 65535:
            raise ValueError('upload_voxels: %d events outside [1, 65535]' % vb.n)
        parts = [(name, getattr(vb, name)) for name in ('offsets', 'index', 'value', 'label', 'weight', 'bg_weight')
                 if getattr(vb, name) is not None]
        at, nbytes = {}, 0
        for name, a in parts:                      # every section starts on a 16-byte boundary
            at[name] = nbytes
            nbytes += (a.nbytes + 15) & ~15
        nbytes = max(nbytes, 16)
        cs = self._copy_stream()
        cur = torch.cuda.current_stream(self._device)
        pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        stage = pinned.numpy()
        for name, a in parts:
            stage[at[name]:at[name] + a.nbytes] = a.view(np.uint8)
        dev = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
        cs.wait_stream(cur)                        # as in _feed: the block may come back with kernels still pending on it
        dev.record_stream(cs)
        with torch.cuda.stream(cs):
            dev.copy_(pinned, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        cur.wait_event(ev)
        ev.synchronize()                           # copy only; kernels of earlier minibatches keep running
        self.feed_stats['h2d_bytes'] += nbytes
        self.feed_stats['h2d_calls'] += 1
        self.feed_stats['staged_bytes'] += nbytes
        res = _DeviceVoxelBatch()
        res.dev, res.big, res.n, res.m = dev, big, vb.n, int(vb.offsets[-1])
        res.offsets, res.index = vb.offsets.copy(), vb.index.copy()
        res.weight = None if vb.weight is None else True      # what _check_make_weight asks: is a weight list there
        res.ptr = {name: dev.data_ptr() + at[name] for name, _ in parts}
        return res

    def _crop_desc(self, big_batch, boxes, dev_boxes, first=0, count=None):
        """``ursn_crop_desc`` over a resident large batch and the run ``[first, first + count)`` of uploaded box arrays."""
        nd = len(self._dims) - 1
        d = _lib.ursn_crop_desc()
        d.ndim, d.n, d.m_total = nd, big_batch.n, big_batch.m
        for i in range(nd):
            d.big[i], d.tile[i] = big_batch.big[i], int(self._dims[i])
        B = len(boxes)
        count = B - first if count is None else count
        d.boxes = count
        for name in ('offsets', 'index', 'value', 'label', 'weight', 'bg_weight'):
            setattr(d, name, big_batch.ptr.get(name))
        # dev_boxes: int32 [B * (1 + nd (+ 2 nd))] = event | origin | core_lo | core_hi
        base = dev_boxes.data_ptr()
        d.box_event = base + 4 * first
        d.box_origin = base + 4 * (B + first * nd)
        if boxes.core_lo is not None:
            d.core_lo = base + 4 * (B + B * nd + first * nd)
            d.core_hi = base + 4 * (B + 2 * B * nd + first * nd)
        return d

    def _upload_boxes(self, boxes, what):
        import torch
        from .tiling import Boxes
        if not isinstance(boxes, Boxes):
            raise ValueError('%s: boxes = %r, expected a tiling.Boxes' % (what, boxes))
        if boxes.ndim != len(self._dims) - 1:
            raise ValueError('%s: boxes of %d axes for a network of %d' % (what, boxes.ndim, len(self._dims) - 1))
        if not 1 <= len(boxes) <= 1 << 20:
            raise ValueError('%s: %d boxes outside [1, 2^20]' % (what, len(boxes)))
        parts = [boxes.event, boxes.origin.reshape(-1)]
        if boxes.core_lo is not None:
            parts += [boxes.core_lo.reshape(-1), boxes.core_hi.reshape(-1)]
        return torch.from_numpy(np.concatenate(parts)).to(self._device)

    def _crop_scratch(self, d):
        import torch
        need = int(_lib.load().ursn_crop_scratch_bytes(d.ndim, d.big, d.tile, d.boxes))
        if need == 0:
            raise ValueError('tiling: shapes big = %r, tile = %r, %d boxes are out of domain'
                             % (list(d.big)[:d.ndim], list(d.tile)[:d.ndim], d.boxes))
        scratch = getattr(self, '_crop_scratch_buf', None)
        if scratch is None or scratch.numel() * 8 < need:
            scratch = self._crop_scratch_buf = torch.empty((need + 7) // 8, dtype=torch.int64, device=self._device)
        return scratch

    def _crop_source(self, voxels, crop, what):
        """The refusals of ``crop=(big_batch, boxes)``; returns the resident large batch, which stands in for ``voxels``."""
        from .tiling import Boxes
        if voxels is not None:
            raise ValueError('%s: crop cuts the minibatch out of the resident batch; voxels must be None' % what)
        if not (isinstance(crop, (tuple, list)) and len(crop) == 2 and isinstance(crop[0], _DeviceVoxelBatch)
                and isinstance(crop[1], Boxes)):
            raise ValueError('%s: crop = %r, expected (upload_voxels(...), tiling.Boxes)' % (what, crop))
        if len(crop[1]) > 65535:
            raise ValueError('%s: %d boxes make a minibatch of more than 65535 events' % (what, len(crop[1])))
        return crop[0]

    def _feed_crop(self, big_batch, boxes, sess, with_label=True, with_weight=None, symmetry=None):
        """``_feed_voxels`` for a crop: the minibatch (one event per box) is written on the device by ``ursn_crop_write`` into a
        list buffer of its own and expanded by ``_expand_voxel_list`` like a fed list.  No count comes back to the host: the
        buffers hold as many entries as the boxes' events have (a box holds no more than its event), capped at a full tile."""
        import torch
        if with_weight is None:
            with_weight = self._use_weight
        if with_weight and 'weight' not in big_batch.ptr:
            sys.stderr.write('Network configured to use loss pixel-weighting. Cannot run w/ weight=None...\n')
            raise TypeError
        if with_label and 'label' not in big_batch.ptr:
            raise ValueError('_feed_crop: the resident batch has no label list')
        dev_boxes = self._upload_boxes(boxes, 'crop')
        d = self._crop_desc(big_batch, boxes, dev_boxes)
        scratch = self._crop_scratch(d)
        B, V = len(boxes), self._label_size
        per_event = np.diff(big_batch.offsets)
        ev = boxes.event.astype(np.int64)
        ok = (ev >= 0) & (ev < big_batch.n)
        cap = int(np.minimum(per_event[np.where(ok, ev, 0)] * ok, V).sum())
        f32 = lambda: torch.empty(max(cap, 1), dtype=torch.float32, device=self._device)
        bufs = {'offsets': torch.empty(B + 1, dtype=torch.int64, device=self._device),
                'index': torch.empty(max(cap, 1), dtype=torch.int32, device=self._device), 'value': f32()}
        if with_label:
            bufs['label'] = f32()
        if with_weight:
            bufs['weight'], bufs['bg_weight'] = f32(), torch.empty(B, dtype=torch.float32, device=self._device)
        o = _lib.ursn_crop_out()
        for name, t in bufs.items():
            setattr(o, name, t.data_ptr())
        o.cap = cap
        _lib.check(_lib.load().ursn_crop_write(ctypes.byref(d), ctypes.byref(o), self._ptr(scratch), scratch.numel() * 8,
                                               self._stream(sess)))
        b = _lib.ursn_voxel_batch()
        b.n, b.voxels = B, V
        for name, t in bufs.items():
            setattr(b, name, t.data_ptr())
        fd = self._expand_voxel_list(b, with_label, with_weight, symmetry)
        cur = torch.cuda.current_stream(self._device)
        for t in list(bufs.values()) + [dev_boxes]:
            t.record_stream(cur)                   # freed with the expansion still pending: the allocator waits for it
        return fd

    def inference_tiled_voxel_scores(self, sess, big_batch, big, halo=0, tile_batch=None, want=('scores', 'pred', 'ana')):
        """``inference_voxel_scores`` for events LARGER than the network: every event of ``big_batch`` (``upload_voxels(vb, big)``,
        or a VoxelBatch at ``prod(big)``, which is uploaded first) is analysed tile by tile with the network's own spatial size as
        the tile, and every listed voxel gets the scores of the ONE tile that owns it.

        1. ``tiling.grid(big, tile, halo)``: boxes at stride ``tile - 2 * halo`` per axis, the last one flush with the end of the
           volume, and cores that partition the volume (the boundary lies in the middle of the overlap of two neighbours);
        2. ``ursn_crop_count`` on the device and ONE small D2H of the per-box counts, the only synchronisation before the forwards;
        3. every box that OWNS no listed voxel is dropped (most tiles of a sparse event);
        4. the rest, in box order, in batches of ``tile_batch`` (None: 4);
        5. per batch ``ursn_crop_write`` (the boxes as a voxel batch at the tile's size), the expansion, forward pass and gather
           head of ``inference_voxel_scores``, then ``ursn_scores_scatter`` of the owned rows to the large event's list order.
        The list goes up once and the scores come back once.  Returns the dict of ``inference_voxel_scores`` (without labels) per
        large event, plus ``tiles_total``, ``tiles_run`` and ``forwards``.

        What tiling is NOT: the network's receptive field exceeds any sensible halo, so the scores of a tiled event are not the
        scores a network built at the large shape would give -- a voxel near a tile's border sees zeros where its neighbours in
        the next tile are.  A larger halo moves the owned voxels away from the borders at the price of more tiles.  With
        batch-statistics BatchNorm (the reference's only mode) a tile's scores also depend on its batch-mates and on how much of
        it is empty, so ``construct(bn_moving=True)`` and ``set_bn_mode('moving')`` are the intended mode: a tile's result then
        depends on the tile alone (up to the reduction order of a batch size, as for any batch)."""
        import torch
        from . import tiling
        self._require_single_channel('inference_tiled_voxel_scores')
        want = tuple(want)
        spec = self._cluster_wanted(want)
        if not want or any(w not in ('scores', 'pred', 'ana') for w in want if spec is None or w != 'cluster'):
            raise ValueError("inference_tiled_voxel_scores: want = %r, expected a non-empty subset of %r"
                             % (want, self._want_names()))
        if 'ana' in want and self._num_class < 3:
            raise ValueError('inference_tiled_voxel_scores: the ana label needs >= 3 classes (num_class = %d)' % self._num_class)
        if tile_batch is not None and int(tile_batch) < 1:
            raise ValueError('inference_tiled_voxel_scores: tile_batch = %r < 1' % (tile_batch,))
        big = tuple(int(s) for s in big)
        matching = spec is not None and getattr(self, '_cluster_matching_on', False)
        if matching and ('label' not in big_batch.ptr if isinstance(big_batch, _DeviceVoxelBatch) else big_batch.label is None):
            raise ValueError('inference_tiled_voxel_scores: cluster matching is on and the batch has no labels to cluster')
        if not isinstance(big_batch, _DeviceVoxelBatch):
            big_batch = self.upload_voxels(big_batch, big)
        if big_batch.big != big:
            raise ValueError('inference_tiled_voxel_scores: the resident batch has shape %r, big = %r' % (big_batch.big, big))
        lib, C, n, M, V = _lib.load(), self._num_class, big_batch.n, big_batch.m, self._label_size
        tile = tuple(int(d) for d in self._dims[:-1])
        boxes = tiling.grid(big, tile, halo, n)
        dev_boxes = self._upload_boxes(boxes, 'inference_tiled_voxel_scores')
        d = self._crop_desc(big_batch, boxes, dev_boxes)
        scratch = self._crop_scratch(d)
        counts = torch.empty((2, len(boxes)), dtype=torch.int64, device=self._device)
        _lib.check(lib.ursn_crop_count(ctypes.byref(d), self._ptr(counts[0]), self._ptr(counts[1]), self._ptr(scratch),
                                       scratch.numel() * 8, self._stream(sess)))
        host_counts = counts.cpu().numpy()
        keep = np.flatnonzero(host_counts[1] > 0)
        kinds = {'scores': ((max(M, 1), C), torch.float32), 'pred': ((max(M, 1),), torch.uint8), 'ana': ((max(M, 1),), torch.uint8)}
        made = [w for w in want if w != 'cluster'] + ([spec.on] if spec is not None and spec.on not in want else [])
        out = {w: torch.zeros(kinds[w][0], dtype=kinds[w][1], device=self._device) for w in made}
        forwards = 0
        if keep.size:
            run = boxes.select(keep)
            per_box = host_counts[0][keep]
            dev_run = self._upload_boxes(run, 'inference_tiled_voxel_scores')
            tb = min(4 if tile_batch is None else int(tile_batch), len(run))
            self._ensure_handle(tb)
            cap = max(int(per_box[i:i + tb].sum()) for i in range(0, len(run), tb))
            i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=self._device)
            bufs = {'offsets': torch.empty(tb + 1, dtype=torch.int64, device=self._device), 'index': i32(cap),
                    'value': torch.empty(max(cap, 1), dtype=torch.float32, device=self._device), 'src': i32(cap),
                    'owned': torch.empty(max(cap, 1), dtype=torch.uint8, device=self._device)}
            rows = {w: torch.empty((max(cap, 1),) + kinds[w][0][1:], dtype=kinds[w][1], device=self._device) for w in made}
            o = _lib.ursn_crop_out()
            for name, t in bufs.items():
                setattr(o, name, t.data_ptr())
            for first in range(0, len(run), tb):
                nb = min(tb, len(run) - first)
                m = int(per_box[first:first + nb].sum())
                dr = self._crop_desc(big_batch, run, dev_run, first, nb)
                o.cap = m
                _lib.check(lib.ursn_crop_write(ctypes.byref(dr), ctypes.byref(o), self._ptr(scratch), scratch.numel() * 8,
                                               self._stream(sess)))
                b = _lib.ursn_voxel_batch()
                b.n, b.voxels = nb, V
                b.offsets, b.index, b.value = o.offsets, o.index, o.value
                fd = self._expand_voxel_list(b, False, False)
                _lib.check(lib.ursn_infer_voxels(self._handle, self._ptr(fd['input_data']), None, nb, ctypes.c_void_p(o.offsets),
                                                 ctypes.c_void_p(o.index), m, self._ptr(rows.get('scores')),
                                                 self._ptr(rows.get('pred')), self._ptr(rows.get('ana')), None, self._stream(sess)))
                _lib.check(lib.ursn_scores_scatter(ctypes.c_void_p(o.src), ctypes.c_void_p(o.owned), m, C,
                                                   self._ptr(rows.get('scores')), self._ptr(rows.get('pred')),
                                                   self._ptr(rows.get('ana')), self._ptr(out.get('scores')),
                                                   self._ptr(out.get('pred')), self._ptr(out.get('ana')), M, self._stream(sess)))
                self._last_feed = fd
                self._mark_consumed(fd)
                forwards += 1
        off = big_batch.offsets
        pending = None
        if spec is not None:                       # behind the last scatter, on the stitched list in the large shape
            pending = self._enqueue_clusters(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], out[spec.on], n, M, big, spec)
        sspec = getattr(self, '_cluster_split_spec', None) if pending is not None else None
        split, base = None, pending                # base: the clustering the records below run on
        if sspec is not None:                      # the stitched list, in the large shape; no table can overflow at M rows
            split = self._enqueue_cluster_split(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], pending[0].data_ptr(), pending[2],
                                                pending[0].data_ptr() + 8 * pending[3], pending[1], n, M, big, sspec, M, M, M)
            if getattr(self, '_cluster_split_downstream', False):
                base = (split[0], split[3], split[8], max(M, 1), n, M)
        objects = None
        if pending is not None and getattr(self, '_cluster_features_on', False):   # the stitched list, in the large shape
            objects = self._enqueue_cluster_features(sess, big_batch.ptr['offsets'], big_batch.ptr['index'],
                                                     big_batch.ptr['value'], base, big)
        pspec = getattr(self, '_cluster_profile_spec', None) if pending is not None else None
        prof = None
        if pspec is not None:                      # the stitched list, in the large shape, behind the object records
            prof_objects = objects if objects is not None else \
                self._enqueue_cluster_features(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], big_batch.ptr['value'],
                                               base, big)
            prof = self._enqueue_cluster_profile(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], big_batch.ptr['value'],
                                                 base, prof_objects, big, pspec, self._profile_bin_cap(M, pspec))
        vspec = getattr(self, '_cluster_vertex_spec', None) if pending is not None else None
        vtx = None
        if vspec is not None:                      # the stitched list, in the large shape: a vertex joins ends from two tiles
            vtx_objects = objects if objects is not None else prof_objects if pspec is not None else \
                self._enqueue_cluster_features(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], big_batch.ptr['value'],
                                               base, big)
            vtx = self._enqueue_cluster_vertices(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], base, vtx_objects,
                                                 base[1], big, vspec, M, self._vertex_inc_cap(M))
        cspec = getattr(self, '_cluster_chain_spec', None) if pending is not None else None
        chain = None
        if cspec is not None:                      # the stitched list, in the large shape: a track cut at a tile seam is joined
            chain_objects = objects if objects is not None else prof_objects if pspec is not None else \
                vtx_objects if vspec is not None else \
                self._enqueue_cluster_features(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], big_batch.ptr['value'],
                                               base, big)
            chain = self._enqueue_cluster_chains(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], base, chain_objects,
                                                 base[1], big, cspec, M)
        nspec = getattr(self, '_cluster_cone_spec', None) if pending is not None else None
        cone = None
        if nspec is not None:                      # the stitched list, in the large shape: a shower crosses tile seams
            cone_objects = objects if objects is not None else prof_objects if pspec is not None else \
                vtx_objects if vspec is not None else chain_objects if cspec is not None else \
                self._enqueue_cluster_features(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], big_batch.ptr['value'],
                                               base, big)
            cone = self._enqueue_cluster_cones(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], base, cone_objects,
                                               base[1], big, nspec, M)
        truth = match = None
        if matching:                               # the large batch's own labels under the same spec, then the match
            at = big_batch.ptr['label'] - big_batch.dev.data_ptr()
            label = big_batch.dev[at:at + 4 * M].view(torch.float32)
            truth = self._enqueue_clusters(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], self._label_classes(label, M),
                                           n, M, big, spec)
            match = self._enqueue_cluster_match(sess, big_batch.ptr['offsets'], pending, truth, big_batch.ptr['value'], n, M, False)
        gspec = getattr(self, '_cluster_graph_spec', None) if pending is not None else None
        graph = None
        if gspec is not None:                      # the stitched list, in the large shape: groups cross tile borders
            graph = self._enqueue_cluster_graph(sess, big_batch.ptr['offsets'], big_batch.ptr['index'], big_batch.ptr['value'],
                                                base[0], base[2], base[1], n, M, big, gspec, M + 1024, True)
        res = {'index': [big_batch.index[off[i]:off[i + 1]].copy() for i in range(n)]}
        for w in want:
            if w == 'cluster':
                continue
            host = out[w][:M].cpu().numpy()
            res[w] = [host[off[i]:off[i + 1]].copy() for i in range(n)]
        if pending is not None:
            res['cluster'], res['clusters'] = self._fetch_clusters(pending, off)
        if split is not None:
            res['split'] = self._fetch_cluster_split(split, off, [int(t['first'].size) for t in res['clusters']])
        src = res['split'] if base is not pending else res      # what the records below describe: the pieces or the components
        if objects is not None:
            res['objects'] = self._fetch_cluster_features(objects, src['clusters'])
        if match is not None:
            res['true_cluster'], res['true_clusters'] = self._fetch_clusters(truth, off)
            res['match'] = self._fetch_cluster_match(match, res['clusters'], res['true_clusters'])
        if graph is not None:
            lists = [big_batch.index[off[i]:off[i + 1]] for i in range(n)]
            res['graph'] = self._finish_cluster_graph(sess, graph, lists, src, gspec, big, value=lambda: self._resident_value(big_batch))
        if prof is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(prof_objects, src['clusters'])
            lists = [big_batch.index[off[i]:off[i + 1]] for i in range(n)]
            res['profiles'] = self._finish_cluster_profile(sess, prof, records, lists, src, pspec, big,
                                                           value=lambda: self._resident_value(big_batch))
        if vtx is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(vtx_objects, src['clusters'])
            lists = [big_batch.index[off[i]:off[i + 1]] for i in range(n)]
            res['vertices'] = self._finish_cluster_vertices(sess, vtx, records, lists, src, vspec, big,
                                                            value=lambda: self._resident_value(big_batch))
        if chain is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(chain_objects, src['clusters'])
            res['chains'] = self._fetch_cluster_chains(chain, records, off)
        if cone is not None:
            records = res['objects'] if objects is not None else self._fetch_cluster_features(cone_objects, src['clusters'])
            res['cones'] = self._fetch_cluster_cones(cone, records, off)
        res['tiles_total'], res['tiles_run'], res['forwards'] = len(boxes), int(keep.size), forwards
        return res

    # ------------------------------------------------------------------------------------------
    # fetch-sets (lib/ssnet.py:91-153)
    # ------------------------------------------------------------------------------------------
    def feed_dict(self, input_data, input_label=None, input_weight=None):
        if input_weight is None and self._use_weight:
            sys.stderr.write('Network configured to use loss pixel-weighting. Cannot run w/ input_weight=None...\n')
            raise TypeError
        fd = {'input_data': self._feed(input_data, self._data_size, 'data')}
        if input_label is not None:
            fd['input_label'] = self._feed(input_label, self._label_size, 'label')
        if input_weight is not None:
            fd['input_weight'] = self._feed(input_weight, self._label_size, 'weight')
        n = fd['input_data'].shape[0]
        for k, v in fd.items():
            if v.shape[0] != n:
                raise ValueError('%s has batch %d, input_data has %d' % (k, v.shape[0], n))
        return fd

    @staticmethod
    def _ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def make_summary(self, sess, input_data, input_label, input_weight=None, normalize_weight=False, make_weight=None):
        """The reference returns a serialized TensorBoard summary; here the three scalars it holds."""
        extra = {} if make_weight is None else {'make_weight': make_weight}
        res, _ = self.run_test(sess, input_data, input_label, input_weight, normalize_weight=normalize_weight, **extra)
        return {'loss': res[0], 'accuracy_all': res[1], 'accuracy_nonzero': res[2]}

    def zero_gradients(self, sess=None):
        if not self._trainable:
            raise RuntimeError('zero_gradients: constructed with trainable=False')
        self._ensure_handle(max(self._max_batch, 1))
        _lib.check(_lib.load().ursn_zero_grad(self._handle, self._stream(sess)))
        return [None]

    def accum_gradients(self, sess, input_data, input_label, input_weight=None, fetch=True, normalize_weight=False,
                        symmetry=None, make_weight=None, loss=None):
        """``normalize_weight`` (not in the reference, whose driver normalises on the host, lib/ssnet_trainval.py:173): the fed
        weights are divided by their per-event sums on the device before the step (``_normalize_fed_weight``); ``input_weight``
        itself, host array or device tensor, is left as it is.  ``symmetry`` (not in the reference, whose users flip and
        transpose on the host): a sequence of one code per event (symmetry.py); the step then sees data, label and weight of event
        i under operation ``symmetry[i]``, permuted on the device (``_apply_symmetry``) before the weight normalisation.  None:
        the call is made exactly as without the keyword.  ``make_weight`` (a weights.WeightSpec; not in the reference, which reads
        the weights as a stored product): ``input_weight`` must be None and no weight crosses PCIe; after the feed and the symmetry
        (over data and label only) ``ursn_make_weights`` makes the weights on the device from the label the step will see, before
        the optional normalisation.  None: the call is made exactly as without the keyword.  ``loss`` (a losses.LossSpec; not in the
        reference, whose one objective is the weighted cross-entropy): the step runs the device loss head (``ursn_accum_step_loss``:
        focal exponent, label smoothing, soft-Dice term) in the place of the plan's head, on the tensors every other keyword left;
        same fetch-set, and ``last_loss_terms()`` then gives the two terms.  None: the call is made exactly as without the
        keyword."""
        if not self._trainable:
            raise RuntimeError('accum_gradients: constructed with trainable=False')
        if make_weight is not None:
            self._check_make_weight(make_weight, input_weight, 'accum_gradients')
            fd = self._feed_for_made_weight(input_data, input_label)
        else:
            fd = self.feed_dict(input_data=input_data, input_label=input_label, input_weight=input_weight)
        if symmetry is not None:
            fd = self._apply_symmetry(fd, symmetry, sess)
        if make_weight is not None:
            self._make_fed_weight(fd, make_weight, sess)
        if normalize_weight:
            self._normalize_fed_weight(fd, sess)
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        out = (ctypes.c_float * 3)()
        w = fd.get('input_weight') if self._use_weight else None
        self._step_call(fd, w, n, out if fetch else None, sess, loss)
        self._bn_track(sess)
        self._last_feed = fd  # keep device inputs alive until the stream has consumed them
        self._mark_consumed(fd)
        doc = ['', 'loss', 'acc. all', 'acc. nonzero']
        if not fetch:
            return None, doc
        return [None, float(out[0]), float(out[1]), float(out[2])], doc

    # ------------------------------------------------------------------------------------------
    # external losses (not in the reference, whose one loss is part of the graph, lib/ssnet.py:57-71): the step cut open at
    # the logits -- logits out, the caller's d(loss)/d(logits) in, gradients ADDED to the flat buffer like accum_gradients'
    # ------------------------------------------------------------------------------------------
    def forward_logits(self, sess, input_data, as_numpy=False):
        """The forward pass of ``accum_gradients`` up to the logits: ``[N, *spatial, num_class]`` fp32, a device tensor by
        default.  The head is not launched (no loss, no accuracies).  ``backward_logits`` may continue this forward as long as
        no other run call comes in between."""
        import torch
        if not self._trainable:
            raise RuntimeError('forward_logits: constructed with trainable=False')
        fd = {'input_data': self._feed(input_data, self._data_size, 'data')}
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        out = torch.empty((n,) + tuple(int(d) for d in self._dims[:-1]) + (self._num_class,), dtype=torch.float32,
                          device=self._device)
        _lib.check(_lib.load().ursn_forward_logits(self._handle, self._ptr(fd['input_data']), n, self._ptr(out),
                                                   self._stream(sess)))
        self._last_feed = fd  # keep the device input alive: backward_logits reads it again (conv0's weight gradient)
        self._mark_consumed(fd)
        return out.cpu().numpy() if as_numpy else out

    def backward_logits(self, sess, dlogits, want_input_grad=False):
        """Backward pass from ``dlogits`` (device tensor or host array, ``[N, *spatial, num_class]``) of the forward the last
        ``forward_logits`` ran; gradients are added to the flat buffer exactly like a step's (``zero_gradients`` /
        ``apply_gradients`` work unchanged).  Returns ``None`` or, with ``want_input_grad``, d(loss)/d(input) ``[N, *dims]`` fp32
        on the device.  Raises when no ``forward_logits`` is pending (another run call came in between, the batch differs)."""
        import torch
        if not self._trainable:
            raise RuntimeError('backward_logits: constructed with trainable=False')
        if self._handle is None or getattr(self, '_last_feed', None) is None:
            raise RuntimeError('backward_logits: no forward_logits has run')
        fd = self._last_feed
        g = dlogits if isinstance(dlogits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(dlogits, dtype=np.float32))
        g = g.detach().to(device=self._device, dtype=torch.float32).contiguous()
        n = int(fd['input_data'].shape[0])
        want = (n,) + tuple(int(d) for d in self._dims[:-1]) + (self._num_class,)
        if tuple(g.shape) != want and tuple(g.shape) != (n, self._label_size * self._num_class):
            raise ValueError('backward_logits: dlogits has shape %s, the pending forward_logits produced %s'
                             % (tuple(g.shape), want))
        din = torch.empty((n,) + tuple(int(d) for d in self._dims), dtype=torch.float32, device=self._device) \
            if want_input_grad else None
        _lib.check(_lib.load().ursn_backward_logits(self._handle, self._ptr(fd['input_data']), self._ptr(g), n, self._ptr(din),
                                                    self._stream(sess)))
        g.record_stream(torch.cuda.current_stream(self._device))
        self._mark_consumed(fd)
        return din

    def accum_gradients_custom(self, sess, input_data, loss_fn, fetch=True):
        """``accum_gradients`` with the caller's objective: ``loss = loss_fn(logits)`` on the logits as a torch autograd leaf
        (``[N, *spatial, num_class]``, device), ``loss.backward()``, then ``backward_logits(logits.grad)``.  Returns
        ``([None, loss], ['', 'loss'])`` (``None`` results with ``fetch=False``: nothing is read back)."""
        logits = self.forward_logits(sess, input_data).requires_grad_(True)
        self._bn_track(sess)
        loss = loss_fn(logits)
        loss.backward()
        self.backward_logits(sess, logits.grad)
        doc = ['', 'loss']
        if not fetch:
            return None, doc
        return [None, float(loss.detach().item())], doc

    # ------------------------------------------------------------------------------------------
    # device loss head (losses.py, loss_head.hip): the ``loss=`` keyword of the step and evaluation calls
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _loss_desc(loss):
        from .losses import LossSpec
        if not isinstance(loss, LossSpec):
            raise TypeError('loss= takes a losses.LossSpec, got %r' % type(loss).__name__)
        return _lib.ursn_loss_desc(loss.gamma, loss.smoothing, loss.dice_weight, loss.dice_eps, loss.ignore_label)

    def _step_call(self, fd, w, n, out, sess, loss):
        """The step of accum_gradients / accum_gradients_voxels: ``ursn_accum_step`` (loss None: today's call, argument for
        argument) or ``ursn_accum_step_loss`` followed by the metrics read the plain call does itself."""
        lib = _lib.load()
        if loss is None:
            _lib.check(lib.ursn_accum_step(self._handle, self._ptr(fd['input_data']), self._ptr(fd['input_label']), self._ptr(w), n, out,
                                           self._stream(sess)))
            return
        d = self._loss_desc(loss)
        _lib.check(lib.ursn_accum_step_loss(self._handle, self._ptr(fd['input_data']), self._ptr(fd['input_label']), self._ptr(w), n,
                                            ctypes.byref(d), self._stream(sess)))
        if out is not None:
            _lib.check(lib.ursn_read_metrics(self._handle, out, self._stream(sess)))

    def _eval_call(self, fd, w, n, out, sess, loss):
        lib = _lib.load()
        if loss is None:
            _lib.check(lib.ursn_eval(self._handle, self._ptr(fd['input_data']), self._ptr(fd['input_label']), self._ptr(w), n, out,
                                     self._stream(sess)))
            return
        d = self._loss_desc(loss)
        _lib.check(lib.ursn_eval_loss(self._handle, self._ptr(fd['input_data']), self._ptr(fd['input_label']), self._ptr(w), n,
                                      ctypes.byref(d), self._stream(sess)))
        _lib.check(lib.ursn_read_metrics(self._handle, out, self._stream(sess)))

    def last_loss_terms(self, sess=None):
        """``(ce_term, dice_term)`` of the last step or evaluation that ran with ``loss=``: loss = ce_term + dice_weight * dice_term."""
        if self._handle is None:
            raise RuntimeError('last_loss_terms: no step has run')
        out = (ctypes.c_float * 2)()
        _lib.check(_lib.load().ursn_read_loss_terms(self._handle, out, self._stream(sess)))
        return float(out[0]), float(out[1])

    def last_feed(self):
        """Device-resident tensors of the most recent accum_gradients / inference_labels call (valid until two more
        batches have been fed): lets a caller re-run them (summary) without another host copy."""
        return dict(self._last_feed)

    def read_metrics(self, sess=None):
        out = (ctypes.c_float * 3)()
        _lib.check(_lib.load().ursn_read_metrics(self._handle, out, self._stream(sess)))
        return [float(out[0]), float(out[1]), float(out[2])]

    def apply_gradients(self, sess=None, lr=None):
        """All-reduce over ranks, then Adam.  ``lr`` (None: the constructor's learning rate) is this step's learning rate, what the
        driver's schedule passes.  After ``set_optimizer`` with anything switched on the step is the guarded one
        (``ursn_apply_adam_guarded``: gradient statistics, clip / skip decision and Adam on the stream, no host round trip);
        otherwise it is ``ursn_apply_adam`` exactly as before.  The all-reduce stays first: every rank then reduces the same
        buffer and reaches the same decision, and a NaN on one rank skips the step on all of them."""
        if not self._trainable:
            raise RuntimeError('apply_gradients: constructed with trainable=False')
        self.allreduce_gradients()
        self.allreduce_bn_moving()
        self._ensure_handle(max(self._max_batch, 1))
        step_lr = float(self._opt._lr) if lr is None else float(lr)
        o = getattr(self, '_optimizer', None)
        if o is not None and (o['clip_norm'] > 0 or o['weight_decay'] > 0 or o['skip_nonfinite']):
            self._opt_require_state()
            d = _lib.ursn_opt_desc()
            d.lr, d.clip_norm, d.weight_decay, d.skip_nonfinite = step_lr, o['clip_norm'], o['weight_decay'], int(o['skip_nonfinite'])
            _lib.check(_lib.load().ursn_apply_adam_guarded(self._handle, ctypes.byref(d), self._stream(sess)))
        else:
            _lib.check(_lib.load().ursn_apply_adam(self._handle, step_lr, self._stream(sess)))
        self._last_lr = step_lr
        return [None]

    # ------------------------------------------------------------------------------------------
    # guarded optimiser step (not in the reference, lib/ssnet.py:72-80 applies the summed gradients unseen; numpy statement
    # of the definitions: optim.py)
    # ------------------------------------------------------------------------------------------
    def set_optimizer(self, clip_norm=0., weight_decay=0., skip_nonfinite=False):
        """What ``apply_gradients`` does besides Adam: ``clip_norm`` > 0 scales the gradient so that its global L2 norm does not
        exceed it, ``weight_decay`` > 0 is decoupled AdamW on every tensor of rank > 1 (never BatchNorm beta),
        ``skip_nonfinite`` leaves parameters and Adam slots untouched on a step whose gradient holds a NaN or Inf (the step
        counter still advances; ``last_apply_status`` counts the skips).  With everything off ``apply_gradients`` stays the
        plain call.  Allocates the device state of the statistics pass and attaches it (again after a handle is re-created)."""
        clip_norm, weight_decay = float(clip_norm), float(weight_decay)
        if not self._trainable:
            raise RuntimeError('set_optimizer: constructed with trainable=False')
        if clip_norm != clip_norm or clip_norm < 0 or clip_norm == float('inf'):
            raise ValueError('set_optimizer: clip_norm = %r, expected a finite number >= 0' % (clip_norm,))
        if not 0.0 <= weight_decay < float('inf'):
            raise ValueError('set_optimizer: weight_decay = %r, expected a finite number >= 0' % (weight_decay,))
        self._optimizer = {'clip_norm': clip_norm, 'weight_decay': weight_decay, 'skip_nonfinite': bool(skip_nonfinite)}
        if getattr(self, '_params', None) is not None:
            self._opt_require_state()

    def _opt_require_state(self):
        """The state buffer of ``ursn_opt_attach``: allocated once, attached to the current handle."""
        import torch
        if getattr(self, '_opt_state', None) is not None and self._handle is not None:
            return
        lib = _lib.load()
        if getattr(self, '_opt_state', None) is None:
            need = ctypes.c_int64(0)
            _lib.check(lib.ursn_opt_state_bytes(ctypes.byref(self._cfg), ctypes.byref(need)))
            self._opt_counters = [0, 0]                     # calls / skips of handles that are gone
            state = torch.empty(int(need.value), dtype=torch.uint8, device=self._device)
            if self._handle is not None:
                _lib.check(lib.ursn_opt_attach(self._handle, self._ptr(state), state.numel()))
            self._opt_state = state
        if self._handle is None:
            self._ensure_handle(max(self._max_batch, 1))    # attaches

    def _opt_carry_counters(self):
        """Before a handle is destroyed: attaching the state to its successor zeroes the cumulative counters, keep them here."""
        if getattr(self, '_opt_state', None) is None or self._handle is None:
            return
        st = _lib.ursn_opt_status()
        _lib.check(_lib.load().ursn_opt_read(self._handle, ctypes.byref(st), None, self._stream(None)))
        self._opt_counters[0] += int(st.calls)
        self._opt_counters[1] += int(st.skipped_total)

    def grad_stats(self, sess, with_param_norms=True):
        """Per-tensor statistics of the flat gradient buffer as it stands (after ``accum_gradients``; after ``apply_gradients`` it
        still holds the step's summed gradient), reduced on the device in one pass: a dict keyed by the TF variable names with
        ``grad_norm`` / ``grad_sumsq`` / ``grad_maxabs`` / ``nonfinite`` and, with ``with_param_norms``, ``param_norm`` /
        ``param_sumsq`` of the weights (else 0.0), plus ``'global'`` = ``grad_norm`` / ``grad_sumsq`` / ``nonfinite``.  Non-finite
        elements count and contribute nothing to the sums (optim.grad_stats_numpy is the definition).  Synchronises.  It
        rewrites the decision fields of ``last_apply_status`` (coef 1, skip 0); the cumulative counters stay."""
        if not self._trainable:
            raise RuntimeError('grad_stats: constructed with trainable=False')
        self._opt_require_state()
        lib, nt = _lib.load(), len(self._specs)
        _lib.check(lib.ursn_grad_stats(self._handle, int(bool(with_param_norms)), self._stream(sess)))
        st, rows = _lib.ursn_opt_status(), (_lib.ursn_opt_tensor * nt)()
        _lib.check(lib.ursn_opt_read(self._handle, ctypes.byref(st), rows, self._stream(sess)))
        info, out = _lib.ursn_param_info(), {}
        for i in range(nt):
            _lib.check(lib.ursn_param(self._handle, i, ctypes.byref(info)))
            r = rows[i]
            out[info.name.decode()] = {'grad_sumsq': r.g_sumsq, 'grad_norm': math.sqrt(r.g_sumsq), 'grad_maxabs': float(r.g_maxabs),
                                       'nonfinite': int(r.nonfinite), 'param_sumsq': r.p_sumsq, 'param_norm': math.sqrt(r.p_sumsq)}
        out['global'] = {'grad_sumsq': st.sumsq, 'grad_norm': st.norm, 'nonfinite': int(st.nonfinite)}
        return out

    def last_apply_status(self, sess=None):
        """The status record after the last guarded ``apply_gradients``: ``sumsq`` / ``norm`` / ``nonfinite`` of the gradient it saw,
        the ``coef`` it multiplied the gradient by, ``skip`` (1: nothing was written), the cumulative ``calls`` and
        ``skipped_total`` of guarded steps since ``set_optimizer``, and ``lr``, the learning rate of the last ``apply_gradients``.
        Synchronises: the only way the host learns of a skip."""
        self._opt_require_state()
        st = _lib.ursn_opt_status()
        _lib.check(_lib.load().ursn_opt_read(self._handle, ctypes.byref(st), None, self._stream(sess)))
        return {'sumsq': st.sumsq, 'norm': st.norm, 'nonfinite': int(st.nonfinite), 'coef': float(st.coef), 'skip': int(st.skip),
                'calls': int(st.calls) + self._opt_counters[0], 'skipped_total': int(st.skipped_total) + self._opt_counters[1],
                'lr': getattr(self, '_last_lr', None)}

    def allreduce_gradients(self):
        """Data parallelism (not in the reference): every rank accumulated its own minibatches, the
        flat gradient buffer is SUMMED over ranks -- the same reduction as assign_add over
        NUM_MINIBATCHES (lib/ssnet.py:77) -- so N ranks == NUM_MINIBATCHES=N on one device."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self._grads, op=dist.ReduceOp.SUM)

    def allreduce_bn_moving(self):
        """Data parallelism: each rank folded its own minibatches' statistics in; the moving buffers are summed over ranks and
        scaled by ``1 / world`` (one fp32 multiply), so that ranks stay identical like the weights do.  No-op without tracking,
        with one rank, or in ``'frozen'`` mode (the buffer does not change there)."""
        import torch.distributed as dist
        if getattr(self, '_bn_buf', None) is None or not self._bn_tracking:
            return
        if self._bn_mode == 'frozen':   # constant, identical on every rank: summing and scaling it would only round it
            return
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self._bn_buf, op=dist.ReduceOp.SUM)
            self._bn_buf.mul_(1.0 / dist.get_world_size())

    # ------------------------------------------------------------------------------------------
    # BatchNorm moving statistics (slim.batch_norm's moving_mean / moving_variance, which the reference never updates nor
    # reads: SURVEY.md Appendix B-3b/c)
    # ------------------------------------------------------------------------------------------
    def _bn_require(self, what):
        if getattr(self, '_bn_buf', None) is None:
            raise RuntimeError('%s: no moving statistics (construct(bn_moving=True) allocates them)' % what)

    def _bn_track(self, sess):
        """One ``assign_moving_average`` of every layer after a training forward (one per minibatch, as UPDATE_OPS would)."""
        if getattr(self, '_bn_buf', None) is not None and self._bn_tracking and self._bn_mode != 'frozen':
            _lib.check(_lib.load().ursn_bn_update(self._handle, 1.0 - self._bn_decay, self._stream(sess)))

    def reset_bn_moving(self):
        """slim's initial values: moving_mean 0, moving_variance 1."""
        import torch
        self._bn_require('reset_bn_moving')
        host = np.zeros(self._bn_size, np.float32)
        for _, c, off in self._bn_specs:
            host[off + c:off + 2 * c] = 1.0
        self._bn_buf.copy_(torch.from_numpy(host))

    def bn_mode(self):
        return self._bn_mode

    def set_bn_mode(self, mode):
        """``'batch'`` (default): every forward normalises with the statistics of the batch it is given, as the reference does.
        ``'moving'``: the forward-only calls (``inference*``, ``run_test*``) normalise with the moving statistics, so an event's
        result no longer depends on its batch; ``accum_gradients*``, ``forward_logits`` and ``backward_logits`` are refused.
        ``'frozen'``: as ``'moving'`` for the forward-only calls, and the training entries run too (``accum_gradients``,
        ``accum_gradients_voxels``, ``accum_gradients_custom``, ``forward_logits`` / ``backward_logits``, ``UResNetFunction``):
        fine-tuning on fixed statistics, with the derivative that treats mean / rstd as constants (``dz = rstd * g``).  The moving
        buffer is neither updated per minibatch nor all-reduced in this mode; weights and beta train as usual."""
        if mode not in ('batch', 'moving', 'frozen'):
            raise ValueError("set_bn_mode: mode must be 'batch', 'moving' or 'frozen', got %r" % (mode,))
        if mode == 'moving':
            self._bn_require("set_bn_mode('moving')")
        if mode == 'frozen' and getattr(self, '_bn_buf', None) is None:
            raise _NoMovingStatistics("set_bn_mode('frozen'): no moving statistics (construct(bn_moving=True) allocates them)")
        if self._handle is not None and getattr(self, '_bn_buf', None) is not None:
            lib = _lib.load()
            _lib.check(lib.ursn_bn_set_frozen(self._handle, int(mode != 'batch')))   # off clears the training switch as well
            if mode != 'batch':
                _lib.check(lib.ursn_bn_frozen_train(self._handle, int(mode == 'frozen')))
        self._bn_mode = mode

    def bn_calibrate(self, sess, batches, reset=True):
        """Usable moving statistics for a checkpoint that has none (the reference's own snapshots hold the initial 0 / 1):
        forward-only over ``batches`` (an iterable of ``input_data``) in batch mode, folding the k-th batch in with momentum
        ``1 / k``, so the buffer ends as the cumulative mean of the batches' statistics.  Returns the number of batches; the
        mode is left as it was found.  Every batch ends in the stream synchronisation ``ursn_infer_voxels`` / ``ursn_infer`` make."""
        import torch
        self._bn_require('bn_calibrate')
        lib, mode = _lib.load(), self._bn_mode
        self.set_bn_mode('batch')
        try:
            if reset:
                self.reset_bn_moving()
            k = 0
            dummy = torch.empty(16, dtype=torch.uint8, device=self._device)
            none = None
            for data in batches:
                fd = {'input_data': self._feed(data, self._data_size, 'data')}
                n = int(fd['input_data'].shape[0])
                self._ensure_handle(n)
                if none is None or none.numel() < n + 1:   # an empty voxel list: n + 1 zero offsets (the index is never read)
                    none = torch.zeros(n + 1, dtype=torch.int64, device=self._device)
                if int(self._dims[-1]) == 1:   # the forward alone: an empty voxel list launches no head at all
                    _lib.check(lib.ursn_infer_voxels(self._handle, self._ptr(fd['input_data']), None, n, self._ptr(none),
                                                     self._ptr(none), 0, None, self._ptr(dummy), None, None, self._stream(sess)))
                else:
                    sm = torch.empty((n, self._label_size * self._num_class), dtype=torch.float32, device=self._device)
                    _lib.check(lib.ursn_infer(self._handle, self._ptr(fd['input_data']), None, n, self._ptr(sm), None,
                                              self._stream(sess)))
                k += 1
                _lib.check(lib.ursn_bn_update(self._handle, 1.0 / k, self._stream(sess)))
                self._last_feed = fd
                self._mark_consumed(fd)
        finally:
            self.set_bn_mode(mode)
        return k

    def bn_moving_names(self):
        return [n + s for n, _, _ in self._bn_specs for s in ('/moving_mean', '/moving_variance')]

    def get_bn_moving(self):
        """{'UResNet/<scope>/BatchNorm/moving_mean' | '.../moving_variance': float32 [cout]}: the TF checkpoint names."""
        self._bn_require('get_bn_moving')
        host = self._bn_buf.detach().cpu().numpy()
        out = {}
        for name, c, off in self._bn_specs:
            out[name + '/moving_mean'] = host[off:off + c].copy()
            out[name + '/moving_variance'] = host[off + c:off + 2 * c].copy()
        return out

    def set_bn_moving(self, values, strict=True):
        """Names and shapes are checked like ``set_variables`` does (``strict``: a missing name is a KeyError, else it keeps its
        value); a negative or non-finite variance (or a non-finite mean) is refused.  Nothing is written unless all pass."""
        import torch
        todo = []
        for name, c, off in self._bn_specs:
            for k, suffix in enumerate(('/moving_mean', '/moving_variance')):
                key = name + suffix
                if key not in values:
                    if strict:
                        raise KeyError(key)
                    continue
                v = np.asarray(values[key], dtype=np.float32)
                if tuple(v.shape) != (c,):
                    raise ValueError('%s: shape %s, expected %s' % (key, v.shape, (c,)))
                if not np.all(np.isfinite(v)) or (k == 1 and np.any(v < 0)):
                    raise ValueError('%s: %s values are refused' % (key, 'negative or non-finite' if k else 'non-finite'))
                todo.append((off + k * c, v))
        self._bn_require('set_bn_moving')
        host = self._bn_buf.detach().cpu().numpy().copy()
        for at, v in todo:
            host[at:at + v.size] = v
        self._bn_buf.copy_(torch.from_numpy(host))

    def run_test(self, sess, input_data, input_label, input_weight=None, normalize_weight=False, make_weight=None, loss=None):
        if make_weight is not None:
            self._check_make_weight(make_weight, input_weight, 'run_test')
            fd = self._feed_for_made_weight(input_data, input_label)
            self._make_fed_weight(fd, make_weight, sess)
        else:
            fd = self.feed_dict(input_data=input_data, input_label=input_label, input_weight=input_weight)
        if normalize_weight:
            self._normalize_fed_weight(fd, sess)
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        out = (ctypes.c_float * 3)()
        w = fd.get('input_weight') if self._use_weight else None
        self._eval_call(fd, w, n, out, sess, loss)
        return [float(out[0]), float(out[1]), float(out[2])], ['loss', 'acc. all', 'acc. nonzero']

    def inference(self, sess, input_data, input_label=None, as_numpy=True):
        import torch
        fd = {'input_data': self._feed(input_data, self._data_size, 'data')}
        if input_label is not None:
            fd['input_label'] = self._feed(input_label, self._label_size, 'label')
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        sm = torch.empty((n,) + tuple(int(d) for d in self._dims[:-1]) + (self._num_class,), dtype=torch.float32,
                         device=self._device)
        out = (ctypes.c_float * 2)()
        _lib.check(_lib.load().ursn_infer(self._handle, self._ptr(fd['input_data']), self._ptr(fd.get('input_label')),
                                          n, self._ptr(sm), out, self._stream(sess)))
        res = [sm.cpu().numpy() if as_numpy else sm]
        if input_label is not None:
            res += [float(out[0]), float(out[1])]
        return res

    def inference_labels(self, sess, input_data, input_label=None, as_numpy=True, with_softmax=False):
        """ana_step's shower/track label volume computed on the device (lib/ssnet_trainval.py:285-287): returns
        [labels [N, *spatial] float32 (, acc_all, acc_nonzero if input_label is given)]; the softmax only leaves the
        kernel when ``with_softmax`` asks for it (appended last, same forward pass)."""
        import torch
        fd = {'input_data': self._feed(input_data, self._data_size, 'data')}
        if input_label is not None:
            fd['input_label'] = self._feed(input_label, self._label_size, 'label')
        n = int(fd['input_data'].shape[0])
        self._ensure_handle(n)
        sp = tuple(int(x) for x in self._dims[:-1])
        out = torch.empty((n,) + sp, dtype=torch.float32, device=self._device)
        sm = torch.empty((n,) + sp + (self._num_class,), dtype=torch.float32, device=self._device) if with_softmax else None
        acc = (ctypes.c_float * 2)()
        _lib.check(_lib.load().ursn_infer_labels(self._handle, self._ptr(fd['input_data']), self._ptr(fd.get('input_label')),
                                                 n, self._ptr(out), self._ptr(sm), acc, self._stream(sess)))
        self._last_feed = fd
        self._mark_consumed(fd)
        res = [out.cpu().numpy() if as_numpy else out]
        if input_label is not None:
            res += [float(acc[0]), float(acc[1])]
        if with_softmax:
            res.append(sm.cpu().numpy() if as_numpy else sm)
        return res

    def _infer_stats(self, sess, fd, with_labels, with_softmax, as_numpy):
        import torch
        n, C = int(fd['input_data'].shape[0]), self._num_class
        self._ensure_handle(n)
        sp = tuple(int(x) for x in self._dims[:-1])
        dev = self._device
        conf = torch.empty((n, C, C), dtype=torch.int64, device=dev)
        other = torch.empty((n, 2), dtype=torch.int64, device=dev)
        nonzero = torch.empty((n, 2), dtype=torch.int64, device=dev) if int(self._dims[-1]) == 1 else None
        ssum = torch.empty((n, C), dtype=torch.float64, device=dev)
        ssq = torch.empty((n, C), dtype=torch.float64, device=dev)
        out = _lib.ursn_class_stats_out()
        out.conf, out.other, out.score_sum, out.score_sq = conf.data_ptr(), other.data_ptr(), ssum.data_ptr(), ssq.data_ptr()
        out.nonzero = nonzero.data_ptr() if nonzero is not None else None
        labels = torch.empty((n,) + sp, dtype=torch.float32, device=dev) if with_labels else None
        sm = torch.empty((n,) + sp + (C,), dtype=torch.float32, device=dev) if with_softmax else None
        dense = with_labels or with_softmax
        acc = (ctypes.c_float * 2)()
        _lib.check(_lib.load().ursn_infer_stats(self._handle, self._ptr(fd['input_data']), self._ptr(fd['input_label']), n,
                                                self._ptr(labels), self._ptr(sm), acc if dense else None, ctypes.byref(out),
                                                self._stream(sess)))
        self._last_feed = fd
        self._mark_consumed(fd)
        res = class_stats_from_counts(conf.cpu().numpy(), other.cpu().numpy(), ssum.cpu().numpy(), ssq.cpu().numpy(),
                                      nonzero.cpu().numpy() if nonzero is not None else None)
        if with_labels:
            res['labels'] = labels.cpu().numpy() if as_numpy else labels
        if with_softmax:
            res['softmax'] = sm.cpu().numpy() if as_numpy else sm
        if dense:
            res['acc_all_batch'], res['acc_nonzero_batch'] = float(acc[0]), float(acc[1])
        return res

    def inference_stats(self, sess, input_data, input_label, with_labels=False, with_softmax=False, as_numpy=True):
        """Per-event, per-class analysis statistics (example_scripts/ana_csv.py:67-116) from ONE forward pass, reduced on the
        device from conv2's stored logits by ``ursn_infer_stats``: only a few hundred bytes per event come back.  Returns the dict
        of ``class_stats_from_counts`` (``conf``, ``other``, ``npx``, ``acc_class``, ``score_mean``, ``score_std``, ``acc_all``,
        ``acc_nonzero_label``, ``acc_nonzero_data``).  ``with_labels`` / ``with_softmax`` add the dense outputs of
        ``inference_labels`` from the same pass (``labels``, ``softmax``) and, with either, the batch accuracies it returns
        (``acc_all_batch``, ``acc_nonzero_batch``); without them the dense head is not launched at all."""
        if input_label is None:
            raise ValueError('inference_stats: input_label is required')
        fd = {'input_data': self._feed(input_data, self._data_size, 'data'),
              'input_label': self._feed(input_label, self._label_size, 'label')}
        return self._infer_stats(sess, fd, with_labels, with_softmax, as_numpy)

    def inference_stats_voxels(self, sess, voxels, with_labels=False, with_softmax=False, as_numpy=True):
        """``inference_stats`` fed a VoxelBatch (with a label list), expanded on the device: no dense label crosses PCIe."""
        self._require_single_channel('inference_stats_voxels')
        fd = self._feed_voxels(voxels, with_label=True, with_weight=False)
        return self._infer_stats(sess, fd, with_labels, with_softmax, as_numpy)

    # ------------------------------------------------------------------------------------------
    # variables (checkpoint / weight injection)
    # ------------------------------------------------------------------------------------------
    def variable_names(self):
        return [s[0] for s in self._specs]

    def get_variables(self):
        host = self._params.detach().cpu().numpy()
        return {name: host[off:off + n].reshape(shape).copy() for name, shape, off, n in self._specs}

    def set_variables(self, values, strict=True):
        import torch
        host = self._params.detach().cpu().numpy().copy()
        for name, shape, off, n in self._specs:
            if name not in values:
                if strict:
                    raise KeyError(name)
                continue
            v = np.asarray(values[name], dtype=np.float32)
            if tuple(v.shape) != tuple(shape):
                raise ValueError('%s: shape %s, expected %s' % (name, v.shape, shape))
            host[off:off + n] = v.reshape(-1)
        self._params.copy_(torch.from_numpy(host))

    def get_gradients(self):
        host = self._grads.detach().cpu().numpy()
        return {name: host[off:off + n].reshape(shape).copy() for name, shape, off, n in self._specs}

    def debug_tensor(self, name):
        """Internal tensor of the last forward/backward as numpy [N, spatial..., C] (parity tests)."""
        import torch
        ptr, vox, ch, cs = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().ursn_tensor(self._handle, name.encode(), ctypes.byref(ptr), ctypes.byref(vox),
                                           ctypes.byref(ch), ctypes.byref(cs)))
        from . import hiprt
        if vox.value == 0:   # <scope>:mean / :rstd -- a per-channel fp32 vector in both precisions
            torch.cuda.synchronize(self._device)
            buf = (ctypes.c_float * ch.value)()
            hiprt.memcpy_d2h(buf, ptr.value, ch.value * 4)
            return np.frombuffer(buf, dtype=np.float32).copy()
        n = self._last_feed['input_data'].shape[0]
        total = int(n * vox.value * cs.value)
        valid = total - (cs.value - ch.value)  # a channel-slice view ends `ch` floats into its last voxel
        torch.cuda.synchronize(self._device)
        bf16 = getattr(self, '_precision', 'fp32') == 'bf16'
        esz = 2 if bf16 else 4
        # one pinned staging buffer per net, grown on demand: a pageable ctypes array cost a memset, a slow copy and a
        # second pass for the contiguous result (1.5 s per 900 MB tensor; the full-size in-situ tests fetch forty of them)
        stage = getattr(self, '_dbg_stage', None)
        if stage is None or stage.numel() < total * esz:
            stage = torch.empty(total * esz, dtype=torch.uint8, pin_memory=True)
            self._dbg_stage = stage
        hiprt.memcpy_d2h(ctypes.c_void_p(stage.data_ptr()), ptr.value, valid * esz)
        raw = stage.numpy()[:total * esz]
        shape = (n,) + tuple(int(d) for d in self._level_dims(int(vox.value))) + (ch.value,)
        if bf16:   # bf16 bit patterns: widen on the host (one pass, into the result)
            a = raw.view(np.uint16).reshape(n, int(vox.value), cs.value)[:, :, :ch.value]
            out = np.empty(shape, dtype=np.float32)
            np.left_shift(a.reshape(shape), 16, out=out.view(np.uint32), dtype=np.uint32, casting='unsafe')
            return out
        a = raw.view(np.float32).reshape(n, int(vox.value), cs.value)[:, :, :ch.value]
        return a.reshape(shape).copy()

    def _level_dims(self, voxels):
        sp = [int(d) for d in self._dims[:-1]]
        while int(np.prod(sp)) > voxels:
            sp = [d // 2 for d in sp]
        return sp

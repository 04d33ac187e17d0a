"""Python 3 driver with the public surface of the reference orchestrator lib/ssnet_trainval.py
(class ssnet_trainval): ``override_config* -> initialize -> batch_process (train_step | ana_step)
-> reset`` (run_ssnet.py:11-19), the same calls into the network object, the same stdout report and
result dictionary.  The body is organised around what this implementation has to get right that
TensorFlow hid: the device never waits for the host.

* a training iteration is ``_IterationPlan`` (which of report / summary / checkpoint fire,
  lib/ssnet_trainval.py:158-161) + ``_run_minibatches`` (zero -> accumulate x NUM_MINIBATCHES ->
  all-reduce + Adam, lib/ssnet_trainval.py:164-191).  Minibatches are launched with ``fetch=False``:
  the H2D copy of minibatch k+1 (pinned buffers, copy stream: ssnet.py::_feed) overlaps the kernels
  of minibatch k, and the three metric scalars are only read back on iterations that report them;
* the ana path writes the shower/track label volume computed on the device
  (lib/ssnet_trainval.py:285-287 -> ursn_infer_labels); the full softmax only crosses PCIe when the
  caller asked for it (``batch_mode=False`` returns it, as the reference does);
* input comes from ``synthetic_io.synthetic_threadio`` (larcv2 / ROOT are not available); ``tf.Session``
  -> ``HipSession``; TensorBoard summaries -> one JSON line per summary step under LOGDIR;
  ``tf.train.Saver`` -> ``.npz`` snapshots keyed by the TF variable names (SAVE_FILE-<iteration>.npz),
  resume parses the iteration from the file name like the reference (lib/ssnet_trainval.py:41-42,139-151);
* data parallelism (absent in the reference): under torch.distributed every rank reads its own entries,
  gradients are summed inside ``apply_gradients`` and reported metrics are averaged over ranks; only
  rank 0 prints, logs and saves.
"""
from __future__ import print_function

import collections
import datetime
import glob
import json
import os
import sys
import time

import numpy as np

from . import optim, symmetry, tiling
from .config import ssnet_config
from .ssnet import HipSession, ana_csv_header, ana_csv_row, graph_csv_header, graph_csv_row, match_csv_header, match_csv_row, objects_csv_header, objects_csv_row, chains_csv_header, chains_csv_row, cones_csv_header, cones_csv_row, split_csv_header, split_csv_row, profiles_csv_header, profiles_csv_row, vertices_csv_header, vertices_csv_row
from .synthetic_io import synthetic_threadio
from .uresnet import uresnet
from .weights import WeightSpec


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist
    except Exception:
        pass
    return None


def _is_rank0():
    d = _dist()
    return d is None or d.get_rank() == 0


_IterationPlan = collections.namedtuple('_IterationPlan', 'iteration report summary checkpoint')


class _ScalarLog(object):
    """Replaces tf.summary.FileWriter (lib/ssnet_trainval.py:118-127): JSON lines under LOGDIR/<sub>/."""

    def __init__(self, logdir, sub):
        os.makedirs(os.path.join(logdir, sub), exist_ok=True)
        self._f = open(os.path.join(logdir, sub, 'scalars.jsonl'), 'a')

    def add_summary(self, summary, iteration):
        rec = dict(summary)
        rec['iteration'] = iteration
        self._f.write(json.dumps(rec) + '\n')
        self._f.flush()

    def close(self):
        self._f.close()


class ssnet_trainval(object):

    def __init__(self):
        self._cfg = ssnet_config()
        self._input_main = None
        self._input_test = None
        self._output = None
        self._csv = None
        self._objects = None
        self._match = None
        self._graph = None
        self._profiles = None
        self._vertices = None
        self._chains = None
        self._cones = None
        self._split = None
        self._iteration = -1
        self._sess = None
        self._net = None
        self._writer_train = self._writer_test = None
        self._weight_spec = None
        self._loss_terms = None

    def __del__(self):
        try:
            self.reset()
        except Exception:
            pass

    # ---- small public helpers of the reference -----------------------------------------------------------
    def _report(self, metrics, descr):
        """lib/ssnet_trainval.py:29-36: 'name=value   ' per documented metric."""
        sys.stdout.write(''.join('%s=%6.6f   ' % (d, m) for m, d in zip(metrics, descr) if d) + '\n')
        sys.stdout.flush()

    def num_class(self):
        return self._cfg.NUM_CLASS

    def iteration_from_file_name(self, file_name):
        stem = file_name[:-4] if file_name.endswith('.npz') else file_name
        return int(stem.rsplit('-', 1)[-1])

    def override_config(self, file_name):
        self._cfg.override(file_name)
        self._cfg.dump()

    def report_memory(self):
        import torch
        return float(torch.cuda.max_memory_allocated())

    def iterations(self):
        return self._cfg.ITERATIONS

    def current_iteration(self):
        return self._iteration

    # ---- initialize (lib/ssnet_trainval.py:51-154) ---------------------------------------------------------
    def _open_stream(self, name, cfg_file, batch):
        io = synthetic_threadio()
        io.configure({'filler_name': name, 'verbosity': 0, 'filler_cfg': cfg_file})
        d = _dist()
        if d is not None and d.get_world_size() > 1:
            io.shard(d.get_rank(), d.get_world_size())   # rank r reads entries r, r+W, r+2W, ...
        if self._cfg.SPARSE_IO:
            io.produce_voxels()
            if self._big_shape():   # ANA_TILE / TRAIN_CROP: the voxel batches hold events of the large shape
                io.produce_large(self._big_shape())
        io.start_manager(batch)
        return io

    def _big_shape(self):
        """The large spatial shape of a tiled run: TRAIN_CROP when training, ANA_TILE when analysing; [] = the keys are off."""
        return list(self._cfg.TRAIN_CROP if self._cfg.TRAIN else self._cfg.ANA_TILE)

    def _advance_main(self):
        keep = not self._cfg.TRAIN
        self._input_main.next(store_entries=keep, store_event_ids=keep)

    def initialize(self):
        cfg = self._cfg
        if not cfg.MAIN_INPUT_CONFIG:
            print('Must provide larcv data filler configuration file!')
            return
        if cfg.ANA_CSV and not cfg.TRAIN and cfg.SPARSE_SCORES:
            raise ValueError('ANA_CSV cannot be combined with SPARSE_SCORES: the per-class statistics run over every voxel, '
                             'SPARSE_SCORES returns scores at the listed voxels only')
        if cfg.ANA_TTA and not cfg.TRAIN and cfg.ANA_CSV:
            raise ValueError('ANA_TTA cannot be combined with ANA_CSV: the per-class statistics are reduced on the device from the '
                             'logits of ONE forward pass, a test-time average only exists as scores after several passes')
        if self._big_shape():
            key = 'TRAIN_CROP' if cfg.TRAIN else 'ANA_TILE'
            if not cfg.SPARSE_IO:
                raise ValueError('%s needs SPARSE_IO True: large events travel as voxel lists only' % key)
            if not cfg.TRAIN and (cfg.ANA_CSV or cfg.ANA_TTA):
                raise ValueError('ANA_TILE cannot be combined with ANA_CSV or ANA_TTA: a tiled analysis returns the scores at the '
                                 'listed voxels of the large event')
        self._cluster_spec = None
        if cfg.ANA_CLUSTER and not cfg.TRAIN:
            if cfg.ANA_CSV:
                raise ValueError('ANA_CLUSTER cannot be combined with ANA_CSV: the clusters are formed at the listed voxels of a '
                                 'voxel-list result, the per-class statistics run over every voxel')
            if not (cfg.SPARSE_IO and (cfg.SPARSE_SCORES or cfg.ANA_TILE)):
                raise ValueError('ANA_CLUSTER needs SPARSE_IO True with SPARSE_SCORES True or ANA_TILE: the clusters are formed on '
                                 'the voxel lists those results hold')
            if cfg.ANA_TTA and not cfg.ANA_TILE:
                raise ValueError('ANA_CLUSTER cannot be combined with ANA_TTA in the driver: cluster the averaged result with '
                                 'ssnet_base.cluster_voxels')
            self._cluster_spec = cfg.cluster_spec()
        if cfg.ANA_OBJECTS and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_OBJECTS needs ANA_CLUSTER: the object records are reductions over the members of the clusters')
        if cfg.ANA_MATCH and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_MATCH needs ANA_CLUSTER: the match compares the predicted clusters with those of the true classes')
        if cfg.ANA_GRAPH and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_GRAPH needs ANA_CLUSTER: the interaction groups are components of the graph of the clusters')
        if cfg.ANA_PROFILES and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_PROFILES needs ANA_CLUSTER: the charge profiles run along the axes of the clusters')
        if cfg.ANA_VERTICES and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_VERTICES needs ANA_CLUSTER: the vertices are where the end points of the clusters meet')
        if cfg.ANA_CHAINS and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_CHAINS needs ANA_CLUSTER: the chains join the clusters that are fragments of one track')
        if cfg.ANA_SPLIT and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_SPLIT needs ANA_CLUSTER: the split cuts the clusters at their junctions and kinks')
        if cfg.ANA_CONES and not cfg.TRAIN and not cfg.ANA_CLUSTER:
            raise ValueError('ANA_CONES needs ANA_CLUSTER: the cones gather the clusters that are fragments of one shower')
        self._weight_spec = None
        if cfg.DEVICE_WEIGHTS and cfg.TRAIN:
            if not cfg.USE_WEIGHTS:
                raise ValueError('DEVICE_WEIGHTS needs USE_WEIGHTS True')
            self._weight_spec = WeightSpec(cfg.DEVICE_WEIGHTS, cfg.WEIGHT_RADIUS, cfg.WEIGHT_SCALE or None)
            self._weight_spec.scales(cfg.NUM_CLASS)
        self._input_main = self._open_stream('MainIO', cfg.MAIN_INPUT_CONFIG, cfg.MINIBATCH_SIZE)
        if cfg.TEST_INPUT_CONFIG:
            self._input_test = self._open_stream('TestIO', cfg.TEST_INPUT_CONFIG, cfg.TEST_BATCH_SIZE)
        if cfg.ANA_OUTPUT_CONFIG:
            self._output = open(cfg.ANA_OUTPUT_CONFIG, 'ab')   # appended ssnet label volumes (.npy records)
        if cfg.ANA_CSV and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_CSV) or os.path.getsize(cfg.ANA_CSV) == 0
            self._csv = open(cfg.ANA_CSV, 'a')
            if fresh:
                self._csv.write(ana_csv_header(cfg.NUM_CLASS))
                self._csv.flush()
        if cfg.ANA_OBJECTS and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_OBJECTS) or os.path.getsize(cfg.ANA_OBJECTS) == 0
            self._objects = open(cfg.ANA_OBJECTS, 'a')
            if fresh:
                self._objects.write(objects_csv_header())
                self._objects.flush()
        if cfg.ANA_MATCH and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_MATCH) or os.path.getsize(cfg.ANA_MATCH) == 0
            self._match = open(cfg.ANA_MATCH, 'a')
            if fresh:
                self._match.write(match_csv_header())
                self._match.flush()
        if cfg.ANA_GRAPH and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_GRAPH) or os.path.getsize(cfg.ANA_GRAPH) == 0
            self._graph = open(cfg.ANA_GRAPH, 'a')
            if fresh:
                self._graph.write(graph_csv_header())
                self._graph.flush()
        if cfg.ANA_PROFILES and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_PROFILES) or os.path.getsize(cfg.ANA_PROFILES) == 0
            self._profiles = open(cfg.ANA_PROFILES, 'a')
            if fresh:
                self._profiles.write(profiles_csv_header())
                self._profiles.flush()
        if cfg.ANA_VERTICES and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_VERTICES) or os.path.getsize(cfg.ANA_VERTICES) == 0
            self._vertices = open(cfg.ANA_VERTICES, 'a')
            if fresh:
                self._vertices.write(vertices_csv_header())
                self._vertices.flush()
        if cfg.ANA_CHAINS and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_CHAINS) or os.path.getsize(cfg.ANA_CHAINS) == 0
            self._chains = open(cfg.ANA_CHAINS, 'a')
            if fresh:
                self._chains.write(chains_csv_header())
                self._chains.flush()
        if cfg.ANA_SPLIT and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_SPLIT) or os.path.getsize(cfg.ANA_SPLIT) == 0
            self._split = open(cfg.ANA_SPLIT, 'a')
            if fresh:
                self._split.write(split_csv_header())
                self._split.flush()
        if cfg.ANA_CONES and not cfg.TRAIN:
            fresh = not os.path.isfile(cfg.ANA_CONES) or os.path.getsize(cfg.ANA_CONES) == 0
            self._cones = open(cfg.ANA_CONES, 'a')
            if fresh:
                self._cones.write(cones_csv_header())
                self._cones.flush()

        # image dimensions come from the first batch, not from the cfg (lib/ssnet_trainval.py:89-93)
        self._advance_main()
        dims = self._input_main.fetch_data(cfg.KEYWORD_DATA).dim()[1:]
        self._net = uresnet(dims=dims, num_class=cfg.NUM_CLASS, base_num_outputs=cfg.BASE_NUM_FILTERS, debug=cfg.DEBUG)
        extra = {'learning_rate': cfg.LEARNING_RATE} if cfg.TRAIN else {}
        ana_moving = not cfg.TRAIN and cfg.ANA_BN == 'moving'
        train_frozen = cfg.TRAIN and cfg.TRAIN_BN == 'frozen'
        if cfg.BN_MOVING or ana_moving or train_frozen:   # default off: construct is then called exactly as before
            extra.update(bn_moving=True, bn_decay=cfg.BN_DECAY)
        self._net.construct(trainable=cfg.TRAIN, use_weight=cfg.USE_WEIGHTS, seed=cfg.TF_RANDOM_SEED,
                            precision=cfg.PRECISION, **extra)
        self._sess = HipSession()
        self._skipped_reported = 0
        if self._cluster_spec is not None:   # default off: never called
            self._net.set_clustering(self._cluster_spec)
            if self._objects:                # default off: never called
                self._net.set_cluster_features(True)
            if self._match:                  # default off: never called
                self._net.set_cluster_matching(True)
            if self._graph:                  # default off: never called
                from .clusters import ClusterGraphSpec
                self._net.set_cluster_graph(ClusterGraphSpec(cfg.GRAPH_GAP))
            if self._profiles:               # default off: never called
                from .clusters import ClusterProfileSpec
                self._net.set_cluster_profiles(ClusterProfileSpec(cfg.PROFILE_STEP, cfg.PROFILE_END_BINS))
            if self._vertices:               # default off: never called
                from .clusters import ClusterVertexSpec
                self._net.set_cluster_vertices(ClusterVertexSpec(cfg.VERTEX_RADIUS, cfg.VERTEX_MIN_SIZE, cfg.VERTEX_CLASSES or None))
            if self._chains:                 # default off: never called
                from .clusters import ClusterChainSpec
                self._net.set_cluster_chains(ClusterChainSpec(cfg.CHAIN_GAP, cfg.CHAIN_MIN_COS, cfg.CHAIN_MIN_SIZE,
                                                              cfg.CHAIN_CLASSES or None, cfg.CHAIN_SAME_CLASS))
            if self._split:                  # default off: never called
                from .clusters import ClusterSplitSpec
                self._net.set_cluster_split(ClusterSplitSpec(cfg.SPLIT_RADIUS, cfg.SPLIT_KINK_COS, cfg.SPLIT_MIN_SIZE,
                                                             cfg.SPLIT_CLASSES or None, None if cfg.SPLIT_GROW < 0 else cfg.SPLIT_GROW),
                                            downstream=cfg.SPLIT_DOWNSTREAM)
            if self._cones:                  # default off: never called
                from .clusters import ClusterConeSpec
                self._net.set_cluster_cones(ClusterConeSpec(cfg.CONE_REACH, cfg.CONE_MIN_COS, cfg.CONE_SEED_SIZE, cfg.CONE_MIN_SIZE,
                                                            cfg.CONE_CLASSES or None, cfg.CONE_SAME_CLASS))
        if cfg.TRAIN and (cfg.CLIP_GRAD_NORM > 0 or cfg.WEIGHT_DECAY > 0 or cfg.SKIP_NONFINITE):   # default off: never called
            self._net.set_optimizer(clip_norm=cfg.CLIP_GRAD_NORM, weight_decay=cfg.WEIGHT_DECAY, skip_nonfinite=cfg.SKIP_NONFINITE)
        bad = [code for code in cfg.ANA_TTA if not symmetry.valid(dims[:-1], code)]
        if bad and not cfg.TRAIN:
            raise ValueError('ANA_TTA: codes %s are not symmetry operations of the image shape %s' % (bad, list(dims[:-1])))

        self._saved = collections.deque()
        if _is_rank0():
            if cfg.LOGDIR:
                self._writer_train = _ScalarLog(cfg.LOGDIR, 'train')
                if self._input_test:
                    self._writer_test = _ScalarLog(cfg.LOGDIR, 'test')
            if cfg.SAVE_FILE:
                save_dir = os.path.dirname(cfg.SAVE_FILE)
                if save_dir:
                    os.makedirs(save_dir, exist_ok=True)
                # snapshots written before a restart take part in the CHECKPOINT_NMAX rotation
                old = glob.glob(glob.escape(cfg.SAVE_FILE) + '-*.npz')
                for path in sorted((p for p in old if p[len(cfg.SAVE_FILE) + 1:-4].isdigit()),
                                   key=self.iteration_from_file_name):
                    self._saved.append(path)
        if cfg.LOAD_FILE:
            self._restore(cfg.LOAD_FILE)
        if ana_moving:
            self._net.set_bn_mode('moving')
        if train_frozen:
            self._net.set_bn_mode('frozen')
        self._descr_metrics = None

    def _restore(self, load_file):
        self._iteration = self.iteration_from_file_name(load_file)
        path = load_file if load_file.endswith('.npz') else load_file + '.npz'
        skip = set(self._cfg.AVOID_LOAD_PARAMS)
        values = {}
        with np.load(path, allow_pickle=False) as f:
            for name in self._net.variable_names():
                if name in skip or (name + ':0') in skip:
                    print('\033[91mSkipping\033[00m loading variable', name, 'from input weight...')
                    continue
                print('\033[95mLoading\033[00m variable', name, 'from', load_file)
                values[name] = f[name]
            moving = {}
            if self._net._bn_buf is not None:   # absent from the file (a snapshot without BN_MOVING): the 0 / 1 stay
                for name in self._net.bn_moving_names():
                    if name not in f.files:
                        continue
                    if name in skip or (name + ':0') in skip:
                        print('\033[91mSkipping\033[00m loading variable', name, 'from input weight...')
                        continue
                    print('\033[95mLoading\033[00m variable', name, 'from', load_file)
                    moving[name] = f[name]
                if not moving:
                    print('\033[91mWarning\033[00m: no BatchNorm moving statistics loaded from %s: they keep their initial 0 / 1' % load_file
                          + (", and ANA_BN 'moving' normalises with those -- the output is meaningless until ssnet_base.bn_calibrate "
                             "(or a BN_MOVING training run) has given the network usable statistics" if self._cfg.ANA_BN == 'moving'
                             and not self._cfg.TRAIN else '')
                          + (", and TRAIN_BN 'frozen' normalises with those -- the training is meaningless until ssnet_base.bn_calibrate "
                             "(or a BN_MOVING training run) has given the network usable statistics" if self._cfg.TRAIN_BN == 'frozen'
                             and self._cfg.TRAIN else ''))
        self._net.set_variables(values, strict=False)
        if moving:
            self._net.set_bn_moving(moving, strict=False)

    # ---- training (lib/ssnet_trainval.py:156-233) ----------------------------------------------------------
    def _plan_iteration(self):
        self._iteration += 1
        it, c = self._iteration, self._cfg
        return _IterationPlan(iteration=it,
                              report=it % c.REPORT_STEPS == 0,
                              summary=bool(c.SUMMARY_STEPS) and it % c.SUMMARY_STEPS == 0,
                              checkpoint=bool(c.CHECKPOINT_STEPS) and (it + 1) % c.CHECKPOINT_STEPS == 0)

    def _pull(self, io, kd, kl, kw):
        """One batch off an IO stream; the per-event weight normalisation mutates the IO buffer in place
        (lib/ssnet_trainval.py:173).  With DEVICE_WEIGHT_NORM the raw weights are handed on and the network call normalises
        them on the device (``normalize_weight=True``); the IO buffer is then not written."""
        data = io.fetch_data(kd).data()
        label = io.fetch_data(kl).data()
        weight = None
        if self._cfg.USE_WEIGHTS and self._weight_spec is None:   # DEVICE_WEIGHTS: made on the device, KEYWORD_WEIGHT is not fetched
            weight = io.fetch_data(kw).data()
            if not self._cfg.DEVICE_WEIGHT_NORM:
                weight /= np.sum(weight, axis=1).reshape([weight.shape[0], 1])
        return data, label, weight

    def _pull_voxels(self, io):
        """SPARSE_IO: the batch as a voxel list; the normalisation of lib/ssnet_trainval.py:173 is done on the list (the sum
        over an event = listed weights + unlisted voxels x background weight, in float64).  With DEVICE_WEIGHT_NORM the list is
        handed on as it is and the expanded dense tensor is normalised on the device."""
        vb = io.fetch_voxels()
        if self._weight_spec is not None:   # DEVICE_WEIGHTS: the weight lists stay on the host
            from .ssnet import VoxelBatch
            return VoxelBatch(vb.offsets, vb.index, vb.value, vb.label, None, None, vb.voxels)
        if self._cfg.USE_WEIGHTS and not self._cfg.DEVICE_WEIGHT_NORM and not self._big_shape():
            vb.normalize_weights()   # TRAIN_CROP: the event that is fed only exists on the device, see _norm_kw
        return vb

    def _norm_kw(self):
        """Keywords of the network calls that are fed what ``_pull`` / ``_pull_voxels`` returned.  Empty with the defaults
        DEVICE_WEIGHT_NORM False and DEVICE_WEIGHTS '': those calls are then made exactly as before."""
        kw = {'normalize_weight': True} if self._cfg.DEVICE_WEIGHT_NORM and self._cfg.USE_WEIGHTS else {}
        if self._big_shape() and self._cfg.USE_WEIGHTS:   # TRAIN_CROP: the sum over a crop can only be taken on the device
            kw['normalize_weight'] = True
        if self._weight_spec is not None:   # DEVICE_WEIGHTS: the call makes the weights from the label it is fed
            kw['make_weight'] = self._weight_spec
        return kw

    def _sym_kw(self, minibatch, n):
        """Keyword of the accumulate calls.  Empty with the default AUGMENT '': those calls are then made exactly as before.  Else
        one symmetry code per event, a function of (AUGMENT_SEED, iteration, minibatch, rank) alone: a resumed run repeats the
        operations, every rank draws its own."""
        c = self._cfg
        if not c.AUGMENT:
            return {}
        d = _dist()
        codes = symmetry.group(c.AUGMENT, [int(x) for x in self._net._dims[:-1]])
        return {'symmetry': symmetry.draw(c.AUGMENT_SEED, self._iteration, minibatch, d.get_rank() if d is not None else 0, n, codes)}

    def _loss_kw(self):
        """Keyword of the accumulate and test calls.  Empty while the LOSS_* keys hold their defaults: those calls are then made
        exactly as before.  Else the device loss head's spec (losses.LossSpec)."""
        spec = self._cfg.loss_spec()
        return {} if spec is None else {'loss': spec}

    def _crop_args(self, vb, minibatch):
        """The ``voxels`` argument and the extra keyword of the ``*_voxels`` calls.  With the default TRAIN_CROP [] the batch
        itself and nothing: those calls are then made exactly as before.  Else the large batch goes up once
        (``upload_voxels``) and the call cuts one crop of the network's size per event out of it on the device; the boxes are a
        function of (CROP_SEED, iteration, minibatch, rank) alone (``minibatch`` -1: the test stream), so a resumed run repeats
        them and every rank draws its own."""
        big = self._big_shape()
        if not big:
            return vb, {}
        d = _dist()
        seed = [int(self._cfg.CROP_SEED), int(self._iteration), int(minibatch) + 1, d.get_rank() if d is not None else 0]
        boxes = tiling.random_boxes(seed, vb, big, [int(x) for x in self._net._dims[:-1]])
        return None, {'crop': (self._net.upload_voxels(vb, big), boxes)}

    def _run_test_voxels(self, test):
        voxels, crop = self._crop_args(test, -1)
        return self._net.run_test_voxels(self._sess, voxels, **self._norm_kw(), **crop, **self._loss_kw())

    def _step_lr(self):
        """The learning rate of the current iteration's optimiser step: what the step is given, the report line prints and the
        summary records.  With a schedule on it is a function of the iteration alone (a resumed run repeats it), else the
        constructor's rate, which the reference's report reads from the optimiser (lib/ssnet_trainval.py:209)."""
        if optim.schedule_on(self._cfg):
            return optim.lr_at(self._cfg, self._iteration)
        return self._net._opt._lr

    def _run_minibatches(self, want_metrics):
        """zero -> NUM_MINIBATCHES x accumulate -> apply.  Returns the per-minibatch metrics [M, 3] when asked for
        (each read is a stream synchronisation), else None; in both cases ``self._last_minibatch`` holds the
        device-resident tensors of the last minibatch for a summary."""
        c, net = self._cfg, self._net
        rows = []
        norm = self._norm_kw()
        norm.update(self._loss_kw())   # the loss comes last in the calls: it sees the tensors every other keyword left
        terms = []
        net.zero_gradients(self._sess)
        for minibatch in range(c.NUM_MINIBATCHES):
            if c.SPARSE_IO:
                vb = self._pull_voxels(self._input_main)
                voxels, crop = self._crop_args(vb, minibatch)
                res, doc = net.accum_gradients_voxels(self._sess, voxels, fetch=want_metrics, **norm, **crop,
                                                      **self._sym_kw(minibatch, vb.n))
            else:
                data, label, weight = self._pull(self._input_main, c.KEYWORD_DATA, c.KEYWORD_LABEL, c.KEYWORD_WEIGHT)
                res, doc = net.accum_gradients(sess=self._sess, input_data=data, input_label=label, input_weight=weight,
                                               fetch=want_metrics, **norm, **self._sym_kw(minibatch, len(data)))
            # the copy has completed, the kernels are queued: the IO may refill this buffer while they run
            self._descr_metrics = doc[1:]
            if want_metrics:
                rows.append(res[1:])
                if 'loss' in norm:
                    terms.append(net.last_loss_terms(self._sess))
            self._advance_main()
        self._last_minibatch = net.last_feed()
        self._loss_terms = np.asarray(terms, np.float64).mean(axis=0) if terms else None   # (ce, dice), mean over the minibatches
        if optim.schedule_on(c):
            net.apply_gradients(self._sess, lr=self._step_lr())
        else:
            net.apply_gradients(self._sess)   # all-reduce(sum) over ranks + Adam
        return np.asarray(rows, np.float32) if want_metrics else None

    def _mean_over_ranks(self, metrics):
        d = _dist()
        if d is None or d.get_world_size() == 1:
            return metrics
        import torch
        dev = self._net._device if d.get_backend() == 'nccl' else 'cpu'
        t = torch.tensor(np.asarray(metrics, np.float64), device=dev)
        d.all_reduce(t, op=d.ReduceOp.SUM)
        return (t / d.get_world_size()).cpu().numpy()

    def train_step(self):
        plan = self._plan_iteration()
        per_minibatch = self._run_minibatches(want_metrics=plan.report)

        test = None
        if (plan.report or plan.summary) and self._input_test:
            c = self._cfg
            self._input_test.next()
            if c.SPARSE_IO:
                test = self._pull_voxels(self._input_test)
            else:
                test = self._pull(self._input_test, c.KEYWORD_TEST_DATA, c.KEYWORD_TEST_LABEL, c.KEYWORD_TEST_WEIGHT)

        gstats = None
        if self._cfg.GRAD_STATS and (plan.report or plan.summary):
            # the report already synchronises.  The status first: grad_stats rewrites its decision fields
            applied = self._net.last_apply_status(self._sess)
            gstats = self._net.grad_stats(self._sess, with_param_norms=plan.summary)
            skipped_since = applied['skipped_total'] - self._skipped_reported
            if plan.report:
                self._skipped_reported = applied['skipped_total']
        if plan.report:
            # report_step is the same on every rank, so the collective inside is safe
            train_mean = self._mean_over_ranks(per_minibatch.mean(axis=0))
            tested = None
            if test is not None:
                norm = self._norm_kw()
                norm.update(self._loss_kw())
                tested = (self._run_test_voxels(test) if self._cfg.SPARSE_IO
                          else self._net.run_test(self._sess, *test, **norm))
            if _is_rank0():
                stamp = datetime.datetime.fromtimestamp(time.time()).strftime('%Y-%m-%d %H:%M:%S')
                sys.stdout.write('@ iteration {:d} LR {:g} Mem {:g} @ {:s}\n'.format(
                    plan.iteration, self._step_lr(), self.report_memory(), stamp))
                sys.stdout.write('Train set: ')
                self._report(train_mean, self._descr_metrics)
                if self._loss_terms is not None:
                    sys.stdout.write('Loss terms: ce=%.6g   dice=%.6g\n' % (self._loss_terms[0], self._loss_terms[1]))
                if gstats is not None:
                    sys.stdout.write('Optimiser: gnorm=%.6g   nonfinite=%d   skipped=%d\n'
                                     % (gstats['global']['grad_norm'], gstats['global']['nonfinite'],
                                        skipped_since))
                if tested is not None:
                    sys.stdout.write('Test set: ')
                    self._report(*tested)
        if plan.summary:
            last = self._last_minibatch   # already normalised, on the host or on the device: never again here
            summ = self._net.make_summary(self._sess, last['input_data'], last['input_label'], last.get('input_weight'))
            lterms = self._loss_terms
            if lterms is None and self._loss_kw():   # a summary without a report: the last minibatch's terms, still on the device
                lterms = self._net.last_loss_terms(self._sess)
            if lterms is not None:
                summ['ce'], summ['dice'] = float(lterms[0]), float(lterms[1])
            if gstats is not None:
                summ['gnorm'] = gstats['global']['grad_norm']
                summ['lr'] = float(self._step_lr())
                summ['skipped_total'] = applied['skipped_total']
                summ['grad_norm'] = {k: v['grad_norm'] for k, v in gstats.items() if k != 'global'}
                summ['weight_norm'] = {k: v['param_norm'] for k, v in gstats.items() if k != 'global'}
            if self._writer_train:
                self._writer_train.add_summary(summ, plan.iteration)
            if self._writer_test and test is not None:
                if self._cfg.SPARSE_IO:
                    t3, _ = self._run_test_voxels(test)
                    tsum = {'loss': t3[0], 'accuracy_all': t3[1], 'accuracy_nonzero': t3[2]}
                else:
                    tsum = self._net.make_summary(self._sess, *test, **self._norm_kw())
                self._writer_test.add_summary(tsum, plan.iteration)
        if plan.checkpoint and self._cfg.SAVE_FILE and _is_rank0():
            print('saved @', self.save_checkpoint())

    def save_checkpoint(self):
        """SAVE_FILE-<iteration>.npz keyed by TF variable names; keeps the newest CHECKPOINT_NMAX files."""
        path = '%s-%d.npz' % (self._cfg.SAVE_FILE, self._iteration)
        arrays = self._net.get_variables()
        if self._cfg.BN_MOVING:
            arrays.update(self._net.get_bn_moving())
        np.savez(path, **arrays)
        if path in self._saved:
            self._saved.remove(path)
        self._saved.append(path)
        while len(self._saved) > max(int(self._cfg.CHECKPOINT_NMAX), 1):
            old = self._saved.popleft()
            if os.path.isfile(old):
                os.remove(old)
        return path

    # ---- analysis (lib/ssnet_trainval.py:235-314) ----------------------------------------------------------
    def ana(self, input_data, input_label=None):
        return self._net.inference(sess=self._sess, input_data=input_data, input_label=input_label)

    def _ana_step_voxels(self, batch_mode):
        """SPARSE_IO ana_step: the event arrives as a voxel list and the record is the voxel set of the label volume -- per
        event ``np.save(index)`` then ``np.save(class)``, the content of the reference's sparse3d product
        (lib/ssnet_trainval.py:299-302).  In batch mode nothing dense crosses PCIe in either direction."""
        from .synthetic_io import voxels_to_dense
        io = self._input_main
        vb = io.fetch_voxels()
        entries = io.fetch_entries()
        if self._cfg.ANA_TILE:
            return self._ana_step_tiled(vb, entries, batch_mode)
        if self._cfg.SPARSE_SCORES:
            return self._ana_step_voxel_scores(vb, entries, batch_mode)
        softmax = data = label = None
        if batch_mode and self._output:
            sets, acc_all, acc_nonzero = self._net.inference_voxels(self._sess, vb, with_labels=True)
        else:
            data, label, _ = voxels_to_dense(vb)
            if self._output:
                labels, acc_all, acc_nonzero, softmax = self._net.inference_labels(self._sess, data, label, with_softmax=True)
                flat = labels.reshape(labels.shape[0], -1)
                sets = [(np.flatnonzero(v).astype(np.int32), v[np.flatnonzero(v)].astype(np.uint8)) for v in flat]
            else:
                softmax, acc_all, acc_nonzero = self.ana(input_data=data, input_label=label)
        if self._output:
            for i, (index, cls) in enumerate(sets):
                print('Entry', entries[i], 'Acc', acc_nonzero)
                np.save(self._output, index)
                np.save(self._output, cls)
            self._output.flush()
        result = None
        if not batch_mode:
            img_shape = list(softmax.shape)
            img_shape[-1] = -1
            result = {'entries': np.array(entries), 'input': data.reshape(img_shape), 'label': label.reshape(img_shape),
                      'softmax': softmax, 'acc_all': acc_all, 'acc_nonzero': acc_nonzero}
        self._advance_main()
        return result

    def _ana_step_voxel_scores(self, vb, entries, batch_mode):
        """SPARSE_IO + SPARSE_SCORES: the output side is a voxel list too (``inference_voxel_scores``), nothing dense is built on
        the host or copied in either direction.  Records per event: ``np.save(index)``, ``np.save(class)`` -- byte for byte those of
        ``_ana_step_voxels`` (the label rule ends in ``* (data > 1.0)``, so the voxel set lies inside the event's list) -- then
        ``np.save(scores[ana != 0])``, the class scores of the voxels in the set, in set order; with ANA_CLUSTER a fourth,
        ``np.save(cluster[ana != 0])``, their cluster ids (and ``cluster`` / ``clusters`` in the per-event dicts).  Interactive mode returns
        ``entries`` / ``acc_all`` / ``acc_nonzero`` and ``voxels``, the per-event list of index / value / label / scores / pred."""
        clustered = getattr(self, '_cluster_spec', None) is not None
        want = ('scores',) + (('ana',) if self._output else ()) + (() if batch_mode else ('pred',)) + (('cluster',) if clustered else ())
        r = self._net.inference_voxel_scores(self._sess, vb, with_labels=True, want=want)
        acc_all, acc_nonzero = r['acc_all'], r['acc_nonzero']
        if self._output:
            for i in range(vb.n):
                keep = r['ana'][i] != 0
                print('Entry', entries[i], 'Acc', acc_nonzero)
                np.save(self._output, r['index'][i][keep])
                np.save(self._output, r['ana'][i][keep])
                np.save(self._output, r['scores'][i][keep])
                if clustered:
                    np.save(self._output, r['cluster'][i][keep])
            self._output.flush()
        self._write_objects(r, entries, vb.offsets, self._net._dims[:-1])
        self._write_match(r, entries)
        self._write_graph(r, entries)
        self._write_profiles(r, entries)
        self._write_vertices(r, entries)
        self._write_chains(r, entries)
        self._write_cones(r, entries)
        self._write_split(r, entries)
        result = None
        if not batch_mode:
            off = vb.offsets
            events = [{'index': r['index'][i], 'value': vb.value[off[i]:off[i + 1]].copy(),
                       'label': vb.label[off[i]:off[i + 1]].copy(), 'scores': r['scores'][i], 'pred': r['pred'][i]}
                      for i in range(vb.n)]
            if clustered:
                for i, ev in enumerate(events):
                    ev['cluster'], ev['clusters'] = r['cluster'][i], r['clusters'][i]
                    if 'objects' in r:
                        ev['objects'] = r['objects'][i]
                    if 'match' in r:
                        ev['true_cluster'], ev['true_clusters'] = r['true_cluster'][i], r['true_clusters'][i]
                    if 'profiles' in r:
                        ev['profiles'] = r['profiles'][i]
                    if 'vertices' in r:
                        ev['vertices'] = r['vertices'][i]
                    if 'chains' in r:
                        ev['chains'] = {'merged': r['chains']['cluster'][i], 'table': r['chains']['clusters'][i],
                                        **r['chains']['events'][i]}
                    if 'cones' in r:
                        ev['cones'] = {'merged': r['cones']['cluster'][i], 'table': r['cones']['clusters'][i],
                                       **r['cones']['events'][i]}
                    if 'split' in r:
                        ev['split'] = {'split': r['split']['cluster'][i], 'table': r['split']['clusters'][i],
                                       **r['split']['events'][i]}
            result = {'entries': np.array(entries), 'acc_all': acc_all, 'acc_nonzero': acc_nonzero, 'voxels': events}
            if 'match' in r:
                result['match'] = r['match']
            if 'graph' in r:
                result['graph'] = r['graph']
        self._advance_main()
        return result

    def _write_objects(self, r, entries, off, shape):
        """ANA_OBJECTS: one CSV row per cluster of every event of the result ``r``."""
        if not getattr(self, '_objects', None) or 'objects' not in r:
            return
        for i, objects in enumerate(r['objects']):
            for k in range(objects['n'].shape[0]):
                self._objects.write(objects_csv_row(entries[i], k, objects, r['index'][i], off[i], shape))
        self._objects.flush()

    def _write_match(self, r, entries):
        """ANA_MATCH: one CSV row per event of the result ``r``."""
        if not getattr(self, '_match', None) or 'match' not in r:
            return
        for i in range(len(entries)):
            self._match.write(match_csv_row(entries[i], r['match']['events'], i))
        self._match.flush()

    def _write_graph(self, r, entries):
        """ANA_GRAPH: one CSV row per interaction group of every event of the result ``r``."""
        if not getattr(self, '_graph', None) or 'graph' not in r:
            return
        for i in range(len(entries)):
            for g in range(int(r['graph'][i]['groups']['rows'].size)):
                self._graph.write(graph_csv_row(entries[i], g, r['graph'][i]['groups']))
        self._graph.flush()

    def _write_profiles(self, r, entries):
        """ANA_PROFILES: one CSV row per cluster of every event of the result ``r``."""
        if not getattr(self, '_profiles', None) or 'profiles' not in r:
            return
        for i in range(len(entries)):
            rows = r['profiles'][i]['rows']
            for k in range(int(rows['bins'].size)):
                self._profiles.write(profiles_csv_row(entries[i], k, rows))
        self._profiles.flush()

    def _write_vertices(self, r, entries):
        """ANA_VERTICES: one CSV row per vertex of every event of the result ``r``."""
        if not getattr(self, '_vertices', None) or 'vertices' not in r:
            return
        for i in range(len(entries)):
            cols = r['vertices'][i]['vertices']
            for k in range(int(cols['ends'].size)):
                self._vertices.write(vertices_csv_row(entries[i], k, cols))
        self._vertices.flush()

    def _write_chains(self, r, entries):
        """ANA_CHAINS: one CSV row per chain of every event of the result ``r``."""
        if not getattr(self, '_chains', None) or 'chains' not in r:
            return
        for i in range(len(entries)):
            cols = r['chains']['events'][i]['chains']
            for k in range(int(cols['rows'].size)):
                self._chains.write(chains_csv_row(entries[i], k, cols))
        self._chains.flush()

    def _write_split(self, r, entries):
        """ANA_SPLIT: one CSV row per junction of every event of the result ``r``."""
        if not getattr(self, '_split', None) or 'split' not in r:
            return
        for i in range(len(entries)):
            cols = r['split']['events'][i]['junctions']
            for k in range(int(cols['row'].size)):
                self._split.write(split_csv_row(entries[i], k, cols))
        self._split.flush()

    def _write_cones(self, r, entries):
        """ANA_CONES: one CSV row per shower of every event of the result ``r``."""
        if not getattr(self, '_cones', None) or 'cones' not in r:
            return
        for i in range(len(entries)):
            cols = r['cones']['events'][i]['showers']
            for k in range(int(cols['rows'].size)):
                self._cones.write(cones_csv_row(entries[i], k, cols))
        self._cones.flush()

    def _ana_step_tiled(self, vb, entries, batch_mode):
        """ANA_TILE: the batch holds events of the large shape; it goes up once and is analysed tile by tile
        (``inference_tiled_voxel_scores``).  Records and the interactive result are those of ``_ana_step_voxel_scores`` with
        indices in the large shape, plus ``tiles`` = (run, total).  Only the listed voxels have scores: ``acc_nonzero`` (over
        data > 0, which all lie in the list) is exact, ``acc_all`` is None."""
        c = self._cfg
        clustered = getattr(self, '_cluster_spec', None) is not None
        want = ('scores', 'pred') + (('ana',) if self._output else ()) + (('cluster',) if clustered else ())
        r = self._net.inference_tiled_voxel_scores(self._sess, vb, c.ANA_TILE, halo=c.ANA_TILE_HALO, tile_batch=c.ANA_TILE_BATCH,
                                                   want=want)
        lit = vb.value > 0
        hit = np.concatenate(r['pred']).astype(np.float32) == vb.label
        acc_all, acc_nonzero = None, float(hit[lit].sum()) / max(int(lit.sum()), 1)
        if self._output:
            for i in range(vb.n):
                keep = r['ana'][i] != 0
                print('Entry', entries[i], 'Acc', acc_nonzero, 'Tiles', r['tiles_run'], 'of', r['tiles_total'])
                np.save(self._output, r['index'][i][keep])
                np.save(self._output, r['ana'][i][keep])
                np.save(self._output, r['scores'][i][keep])
                if clustered:
                    np.save(self._output, r['cluster'][i][keep])
            self._output.flush()
        self._write_objects(r, entries, vb.offsets, c.ANA_TILE)
        self._write_match(r, entries)
        self._write_graph(r, entries)
        self._write_profiles(r, entries)
        self._write_vertices(r, entries)
        self._write_chains(r, entries)
        self._write_cones(r, entries)
        self._write_split(r, entries)
        result = None
        if not batch_mode:
            off = vb.offsets
            events = [{'index': r['index'][i], 'value': vb.value[off[i]:off[i + 1]].copy(),
                       'label': vb.label[off[i]:off[i + 1]].copy(), 'scores': r['scores'][i], 'pred': r['pred'][i]}
                      for i in range(vb.n)]
            if clustered:
                for i, ev in enumerate(events):
                    ev['cluster'], ev['clusters'] = r['cluster'][i], r['clusters'][i]
                    if 'objects' in r:
                        ev['objects'] = r['objects'][i]
                    if 'match' in r:
                        ev['true_cluster'], ev['true_clusters'] = r['true_cluster'][i], r['true_clusters'][i]
                    if 'profiles' in r:
                        ev['profiles'] = r['profiles'][i]
                    if 'vertices' in r:
                        ev['vertices'] = r['vertices'][i]
                    if 'chains' in r:
                        ev['chains'] = {'merged': r['chains']['cluster'][i], 'table': r['chains']['clusters'][i],
                                        **r['chains']['events'][i]}
                    if 'cones' in r:
                        ev['cones'] = {'merged': r['cones']['cluster'][i], 'table': r['cones']['clusters'][i],
                                       **r['cones']['events'][i]}
                    if 'split' in r:
                        ev['split'] = {'split': r['split']['cluster'][i], 'table': r['split']['clusters'][i],
                                       **r['split']['events'][i]}
            result = {'entries': np.array(entries), 'acc_all': acc_all, 'acc_nonzero': acc_nonzero, 'voxels': events,
                      'tiles': (r['tiles_run'], r['tiles_total'])}
            if 'match' in r:
                result['match'] = r['match']
            if 'graph' in r:
                result['graph'] = r['graph']
        self._advance_main()
        return result

    def _ana_step_csv(self, batch_mode):
        """ANA_CSV: ana_step's one forward pass goes through ``inference_stats`` / ``inference_stats_voxels``; the ANA_OUTPUT
        records are those of ``ana_step`` / ``_ana_step_voxels``, one CSV row (example_scripts/ana_csv.py) is appended per entry
        and the interactive result dict also holds ``stats``."""
        from .synthetic_io import voxels_to_dense
        c, io, net = self._cfg, self._input_main, self._net
        want = dict(with_labels=bool(self._output), with_softmax=not batch_mode)
        if c.SPARSE_IO:
            vb = io.fetch_voxels()
            entries = io.fetch_entries()
            on_device = batch_mode and bool(self._output)   # nothing dense crosses PCIe: the voxel set is compacted on the device
            stats = net.inference_stats_voxels(self._sess, vb, as_numpy=not on_device, **want)
            if not batch_mode:
                batch_data, batch_label, _ = voxels_to_dense(vb)
        else:
            batch_data = io.fetch_data(c.KEYWORD_DATA).data()
            batch_label = io.fetch_data(c.KEYWORD_LABEL).data()
            entries = io.fetch_entries()
            stats = net.inference_stats(self._sess, batch_data, batch_label, **want)
        acc_all, acc_nonzero = stats.get('acc_all_batch'), stats.get('acc_nonzero_batch')
        if self._output:
            labels = stats.pop('labels')
            if c.SPARSE_IO:
                if on_device:
                    sets = net.labels_to_voxel_sets(self._sess, labels, int(np.count_nonzero(vb.value > 1.0)))
                else:
                    flat = labels.reshape(labels.shape[0], -1)
                    sets = [(np.flatnonzero(v).astype(np.int32), v[np.flatnonzero(v)].astype(np.uint8)) for v in flat]
                for i, (index, cls) in enumerate(sets):
                    print('Entry', entries[i], 'Acc', acc_nonzero)
                    np.save(self._output, index)
                    np.save(self._output, cls)
            else:
                for i in range(labels.shape[0]):
                    print('Entry', entries[i], 'Acc', acc_nonzero)
                    np.save(self._output, labels[i])
            self._output.flush()
        for i in range(len(entries)):
            self._csv.write(ana_csv_row(entries[i], stats, i))
        self._csv.flush()
        result = None
        if not batch_mode:
            softmax = stats.pop('softmax')
            img_shape = list(softmax.shape)
            img_shape[-1] = -1
            result = {'entries': np.array(entries), 'input': np.array(batch_data).reshape(img_shape),
                      'label': np.array(batch_label).reshape(img_shape), 'softmax': softmax,
                      'acc_all': acc_all, 'acc_nonzero': acc_nonzero, 'stats': stats}
        self._advance_main()
        return result

    def _ana_step_tta(self, batch_mode):
        """ANA_TTA: the scores are the mean over the listed symmetric views of every event, mapped back on the device
        (``inference_tta``; with SPARSE_IO ``inference_voxel_scores_tta``, which gathers every view at the event's own voxels).
        Labels, records and accuracies are formed from the averaged scores by the rules of ``ana_step`` /
        ``_ana_step_voxel_scores``.  With SPARSE_IO only the listed voxels have scores: ``acc_nonzero`` (over data > 0, which
        all lie in the list) is exact, ``acc_all`` is None."""
        c, io, net = self._cfg, self._input_main, self._net
        codes = list(c.ANA_TTA)
        if c.SPARSE_IO:
            vb = io.fetch_voxels()
            entries = io.fetch_entries()
            r = net.inference_voxel_scores_tta(self._sess, vb, codes)
            lit = vb.value > 0
            hit = np.concatenate(r['pred']).astype(np.float32) == vb.label
            acc_all, acc_nonzero = None, float(hit[lit].sum()) / max(int(lit.sum()), 1)
            if self._output:
                for i in range(vb.n):
                    keep = r['ana'][i] != 0
                    print('Entry', entries[i], 'Acc', acc_nonzero)
                    np.save(self._output, r['index'][i][keep])
                    np.save(self._output, r['ana'][i][keep])
                    np.save(self._output, r['scores'][i][keep])
                self._output.flush()
            result = None
            if not batch_mode:
                off = vb.offsets
                events = [{'index': r['index'][i], 'value': vb.value[off[i]:off[i + 1]].copy(),
                           'label': vb.label[off[i]:off[i + 1]].copy(), 'scores': r['scores'][i], 'pred': r['pred'][i]}
                          for i in range(vb.n)]
                result = {'entries': np.array(entries), 'acc_all': acc_all, 'acc_nonzero': acc_nonzero, 'voxels': events}
            self._advance_main()
            return result
        batch_data = io.fetch_data(c.KEYWORD_DATA).data()
        batch_label = io.fetch_data(c.KEYWORD_LABEL).data()
        entries = io.fetch_entries()
        softmax = net.inference_tta(self._sess, batch_data, codes)
        hit = softmax.argmax(axis=-1) == np.asarray(batch_label).reshape(softmax.shape[:-1])
        acc_all, acc_nonzero = float(hit.mean()), None
        if softmax.size == np.asarray(batch_data).size * softmax.shape[-1]:   # one input channel: data > 0 names voxels
            lit = np.asarray(batch_data).reshape(softmax.shape[:-1]) > 0
            acc_nonzero = float(hit[lit].sum()) / max(int(lit.sum()), 1)
        if self._output:
            # lib/ssnet_trainval.py:285-287 on the averaged scores
            shower, track = softmax[..., 1], softmax[..., 2]
            labels = ((shower > track) * 1.0 + (track >= shower) * 2.0) * (np.asarray(batch_data).reshape(shower.shape) > 1.0)
            for i in range(labels.shape[0]):
                print('Entry', entries[i], 'Acc', acc_nonzero)
                np.save(self._output, labels[i].astype(np.float32))
            self._output.flush()
        result = None
        if not batch_mode:
            img_shape = list(softmax.shape)
            img_shape[-1] = -1
            result = {'entries': np.array(entries), 'input': np.array(batch_data).reshape(img_shape),
                      'label': np.array(batch_label).reshape(img_shape), 'softmax': softmax,
                      'acc_all': acc_all, 'acc_nonzero': acc_nonzero}
        self._advance_main()
        return result

    def ana_step(self, batch_mode=False):
        self._iteration += 1
        if self._csv:
            return self._ana_step_csv(batch_mode)
        if self._cfg.ANA_TTA:
            return self._ana_step_tta(batch_mode)
        if self._cfg.SPARSE_IO:
            return self._ana_step_voxels(batch_mode)
        c, io = self._cfg, self._input_main
        batch_data = io.fetch_data(c.KEYWORD_DATA).data()
        batch_label = io.fetch_data(c.KEYWORD_LABEL).data()
        entries = io.fetch_entries()

        softmax = labels = None
        if self._output:
            # the label rule runs inside the head kernel; the softmax is only brought back when it is returned
            out = self._net.inference_labels(self._sess, batch_data, batch_label, with_softmax=not batch_mode)
            labels, acc_all, acc_nonzero = out[0], out[1], out[2]
            if not batch_mode:
                softmax = out[3]
            for i in range(labels.shape[0]):
                print('Entry', entries[i], 'Acc', acc_nonzero)
                np.save(self._output, labels[i])
            self._output.flush()
        else:
            softmax, acc_all, acc_nonzero = self.ana(input_data=batch_data, input_label=batch_label)

        result = None
        if not batch_mode:
            img_shape = list(softmax.shape)
            img_shape[-1] = -1
            result = {'entries': np.array(entries), 'input': np.array(batch_data).reshape(img_shape),
                      'label': np.array(batch_label).reshape(img_shape), 'softmax': softmax,
                      'acc_all': acc_all, 'acc_nonzero': acc_nonzero}
        self._advance_main()
        return result

    def batch_process(self):
        for _ in range(self._cfg.ITERATIONS):
            if self._cfg.TRAIN and self._iteration >= self._cfg.ITERATIONS:
                print('Finished training (iteration %d)' % self._iteration)
                break
            if self._cfg.TRAIN:
                self.train_step()
            else:
                self.ana_step(batch_mode=True)

    def reset(self):
        for attr in ('_input_main', '_input_test'):
            io = getattr(self, attr, None)
            if io is not None:
                io.reset()
                setattr(self, attr, None)
        for attr in ('_output', '_csv', '_objects', '_match', '_graph', '_profiles', '_vertices', '_chains', '_cones', '_split', '_writer_train', '_writer_test'):
            f = getattr(self, attr, None)
            if f is not None:
                f.close()
                setattr(self, attr, None)

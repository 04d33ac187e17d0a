"""Python 3 mirror of the reference flag system (lib/config.py:6-76).

Same class-attribute defaults (lib/config.py:8-36) and the same file format: one ``KEY VALUE``
per line, ``#`` starts a comment, VALUE is a Python literal.  Differences, chosen on purpose
(SURVEY.md Appendix E): values are parsed with ``ast.literal_eval`` instead of ``exec``
(lib/config.py:61,66), and an unknown key is reported and skipped instead of crashing
(lib/config.py:57-61 prints the warning but then fails inside ``exec``), so the shipped
``config/ana3d.cfg`` loads.
"""
from __future__ import print_function

import ast
import os


class ssnet_config(object):

    NUM_CLASS = 3
    BASE_NUM_FILTERS = 16
    MAIN_INPUT_CONFIG = 'config/input_train.cfg'
    TEST_INPUT_CONFIG = ''
    ANA_OUTPUT_CONFIG = ''
    LOGDIR = 'ssnet_train_log'
    SAVE_FILE = 'ssnet_checkpoint/uresnet'
    LOAD_FILE = ''
    AVOID_LOAD_PARAMS = []
    LEARNING_RATE = -1
    MINIBATCH_SIZE = 10
    NUM_MINIBATCHES = 5
    TEST_BATCH_SIZE = 10
    ITERATIONS = 100000
    TF_RANDOM_SEED = 1234
    TRAIN = True
    DEBUG = False
    USE_WEIGHTS = True
    REPORT_STEPS = 200
    SUMMARY_STEPS = 20
    CHECKPOINT_STEPS = 200
    CHECKPOINT_NMAX = 10
    CHECKPOINT_NHOUR = 0.4
    KEYWORD_DATA = 'data'
    KEYWORD_LABEL = 'label'
    KEYWORD_WEIGHT = 'weight'
    KEYWORD_TEST_DATA = ''
    KEYWORD_TEST_LABEL = ''
    KEYWORD_TEST_WEIGHT = ''
    # not in the reference (fp32 TensorFlow): 'fp32' | 'bf16' -- bf16 = mixed precision of BASELINE.json configs[4]
    # (activations / gradient tensors bf16 in HBM, fp32 parameters, statistics, accumulators and Adam)
    PRECISION = 'fp32'
    # not in the reference (larcv fills dense arrays): True = events travel as voxel lists (synthetic_threadio.fetch_voxels ->
    # the *_voxels methods of ssnet_base) and the ana output holds one (index, class) voxel set per event, the content of the
    # sparse3d product of lib/ssnet_trainval.py:299-302, instead of the dense label volume
    SPARSE_IO = False
    # only meaningful with SPARSE_IO: True = the ana output side is a voxel list too (ssnet_base.inference_voxel_scores): class
    # scores, argmax class and ana label come back at the event's own voxels, no dense softmax is written or copied, batch mode
    # appends a third record per event (the class scores of the voxel set) and the interactive result dict holds per-event lists
    SPARSE_SCORES = False
    # not in the reference (lib/ssnet_trainval.py:173,204 normalise the pixel weights per event on the host): True = the driver
    # hands the raw weights on and the network calls divide them by their per-event sums on the device (ursn_normalize_weights:
    # fp64 sum, correctly rounded fp32 division); the IO buffer is then not written.  False = the reference's host pass
    DEVICE_WEIGHT_NORM = False
    # not in the reference (example_scripts/ana_csv.py computes its CSV on the host from the dense softmax): a file name = ana_step
    # makes its one forward pass through ssnet_base.inference_stats* and appends the reference's CSV row per entry (per-event
    # accuracies, per-class pixel count / accuracy / score mean / score std, reduced on the device); '' = off.  Ignored with
    # TRAIN; refused together with SPARSE_SCORES
    ANA_CSV = ''
    # not in the reference (its users flip / transpose the volumes on the host before the feed): '' | 'flip' | 'cube' = every
    # training minibatch is fed through one random symmetry operation per event (symmetry.py: 'flip' the axis flips, 'cube' every
    # flip / axis permutation the image shape admits), applied on the device to data, label and weight alike
    # (ursn_sym_apply, with SPARSE_IO ursn_voxels_to_dense_sym).  The operations are a function of (AUGMENT_SEED, iteration,
    # minibatch, rank) alone, so a resumed run repeats them.  '' = off
    AUGMENT = ''
    AUGMENT_SEED = 0
    # not in the reference: a non-empty list of symmetry codes = ana_step averages the softmax over these views of every event
    # (ssnet_base.inference_tta, with SPARSE_IO inference_voxel_scores_tta); [0] is the plain pass, [] = off.  Ignored with
    # TRAIN; refused together with ANA_CSV
    ANA_TTA = []
    # not in the reference, where slim.batch_norm's moving_mean / moving_variance exist but are never updated nor read
    # (is_training stays True, UPDATE_OPS never run).  BN_MOVING True = every training minibatch folds its batch statistics into
    # the moving statistics with momentum 1 - BN_DECAY (slim's assign_moving_average), checkpoints carry them under the TF names
    # UResNet/<scope>/BatchNorm/moving_mean | moving_variance and a restore loads them when the file has them (else 0 / 1).
    # ANA_BN 'batch' | 'moving' = which statistics the ana driver's forward passes normalise with, in all its output modes;
    # 'moving' makes an event's result independent of the events that share its batch.  Defaults: off, as the reference behaves
    # TRAIN_BN 'batch' | 'frozen' = which statistics the TRAINING steps normalise with.  'frozen' fine-tunes on the loaded moving
    # statistics (small batches, crops, a new sample): forward and backward treat them as constants, the moving buffer is not
    # updated, weights and beta train as usual; it implies the moving buffer (as BN_MOVING allocates it).  Ignored without TRAIN
    BN_MOVING = False
    BN_DECAY = 0.999
    ANA_BN = 'batch'
    TRAIN_BN = 'batch'
    # not in the reference, where the pixel weight is a stored larcv product (config/input_train3d.cfg: Tensor3DProducer "weight")
    # that an upstream module wrote from the label.  DEVICE_WEIGHTS 'class' | 'invfreq' = the train and test steps make the
    # weights on the device from the label (ursn_make_weights; weights.py holds the definition): KEYWORD_WEIGHT is not fetched,
    # no weight crosses PCIe and with SPARSE_IO the weight lists are dropped from the batch.  'class' = WEIGHT_SCALE[category],
    # 'invfreq' = WEIGHT_SCALE[category] / (voxels of the event in that category).  WEIGHT_RADIUS 1..3 = foreground voxels with
    # another foreground class within that Chebyshev distance form a category of their own, the last entry of WEIGHT_SCALE
    # (NUM_CLASS + 1 numbers; [] = all ones).  Needs USE_WEIGHTS; composes with DEVICE_WEIGHT_NORM and AUGMENT.  '' = off
    DEVICE_WEIGHTS = ''
    WEIGHT_RADIUS = 0
    WEIGHT_SCALE = []
    # not in the reference, whose optimiser applies the summed minibatch gradients unseen (lib/ssnet.py:72-80).  All off by default:
    # the step is then the plain Adam call.  CLIP_GRAD_NORM > 0 = the gradient is scaled so that its global L2 norm does not exceed
    # it; WEIGHT_DECAY > 0 = decoupled AdamW on every tensor of rank > 1 (never BatchNorm beta); SKIP_NONFINITE True = a step whose
    # gradient holds a NaN or Inf leaves parameters and Adam slots untouched (decided on the device, ssnet_base.set_optimizer; the
    # step counter still advances).  GRAD_STATS True = summary steps append the global gradient norm and the per-tensor gradient
    # and weight norms to LOGDIR/train/scalars.jsonl and report steps print gnorm= and the steps skipped since the last report.
    # The learning rate is optim.lr_at(iteration): linear warm-up over LR_WARMUP_STEPS iterations from
    # LEARNING_RATE / LR_WARMUP_STEPS, then LEARNING_RATE * LR_DECAY_RATE ** (iteration // LR_DECAY_STEPS); a pure function of the
    # iteration, so a resumed run repeats it
    CLIP_GRAD_NORM = 0.
    WEIGHT_DECAY = 0.
    SKIP_NONFINITE = False
    GRAD_STATS = False
    LR_WARMUP_STEPS = 0
    LR_DECAY_STEPS = 0
    LR_DECAY_RATE = 1.
    # not in the reference, whose network and events share one size.  All off by default and all need SPARSE_IO True; the synthetic
    # IO then produces events of the LARGE shape while the network keeps the image shape of the input configuration.
    # ANA_TILE [large spatial shape] (with TRAIN False) = ana_step uploads every batch once as a voxel list at that shape and
    # analyses it tile by tile (ssnet_base.inference_tiled_voxel_scores: boxes of the network's size at stride tile - 2 *
    # ANA_TILE_HALO, the boxes that own no listed voxel dropped, ANA_TILE_BATCH boxes per forward pass); every listed voxel gets the
    # scores of the one tile that owns it and the output is SPARSE_SCORES' per-event lists.  Tiled scores are not the scores of a
    # network built at the large shape (the receptive field exceeds any halo); ANA_BN 'moving' makes a tile independent of its
    # batch-mates.  Refused together with ANA_CSV and ANA_TTA.  TRAIN_CROP [large spatial shape] (with TRAIN True) = every training
    # and test minibatch is one crop of the network's size per large event, cut out on the device around a listed voxel
    # (tiling.random_boxes, a function of (CROP_SEED, iteration, minibatch, rank) alone, so a resumed run repeats the crops);
    # composes with AUGMENT, DEVICE_WEIGHTS and DEVICE_WEIGHT_NORM.  [] = off
    ANA_TILE = []
    ANA_TILE_HALO = 0
    ANA_TILE_BATCH = 4
    TRAIN_CROP = []
    CROP_SEED = 0
    # not in the reference, whose one objective is the weighted softmax cross-entropy of lib/ssnet.py:57-71.  All off by default: the
    # steps then run the plan's head exactly as before.  Any key set = the train and test steps run the device loss head
    # (losses.py holds the definition): LOSS_FOCAL_GAMMA 0 or >= 1 = the focal exponent on (1 - p_label); LOSS_LABEL_SMOOTHING in
    # [0, 1) = the share of the target spread evenly over the classes; LOSS_DICE_WEIGHT >= 0 = the weight of the batch soft-Dice
    # term (its sums run over the minibatch of ONE rank) with LOSS_DICE_EPS > 0 in numerator and denominator; LOSS_IGNORE_LABEL = a
    # label whose voxels take no part in the loss (-1: none).  Report lines and scalars.jsonl then carry ce= and dice=
    LOSS_FOCAL_GAMMA = 0.
    LOSS_LABEL_SMOOTHING = 0.
    LOSS_DICE_WEIGHT = 0.
    LOSS_DICE_EPS = 1.
    LOSS_IGNORE_LABEL = -1
    # not in the reference, whose users group the predicted voxels into objects on the host.  ANA_CLUSTER 'pred' | 'ana' (with
    # TRAIN False) = ana_step labels the connected components of the argmax class / the ana label at the event's listed voxels on
    # the device (ssnet_base.set_clustering; clusters.py holds the definition): batch mode appends a fourth record per event, the
    # cluster id (-1: none) of every voxel of the set, and the interactive result's per-event dicts gain cluster / clusters.  Needs
    # SPARSE_IO with SPARSE_SCORES or ANA_TILE (tiled: clusters cross tile borders); refused together with ANA_CSV.
    # CLUSTER_CONNECTIVITY 0 = 26 in 3-D and 8 in 2-D, else 6 | 18 | 26 | 4 | 8; CLUSTER_CLASSES [] = every class but 0;
    # CLUSTER_MIN_SIZE = components with fewer voxels get no id.  '' = off.  Ignored with TRAIN, like every ANA_* key; refused
    # together with ANA_TTA (cluster the averaged result with ssnet_base.cluster_voxels instead)
    ANA_CLUSTER = ''
    CLUSTER_CONNECTIVITY = 0
    CLUSTER_CLASSES = []
    CLUSTER_MIN_SIZE = 1
    # ANA_OBJECTS '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per cluster: the object record the device reduces from
    # the cluster's members (ssnet_base.set_cluster_features; clusters.cluster_features_numpy holds the definition): entry, id,
    # class, size, charge, centroid, eigenvalues and principal axis of the covariance, length, and the two end points.  '' = off.
    # Refused without ANA_CLUSTER; ignored with TRAIN, like every ANA_* key
    ANA_OBJECTS = ''
    # ANA_MATCH '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per event: the match of the predicted clusters with the
    # clusters of the TRUE classes under the same CLUSTER_* keys (ssnet_base.set_cluster_matching; clusters.cluster_match_numpy holds
    # the definition): entry, the twelve event integers (matched entries, pair counts, cells, rows, mutual pairs, overlaps) and the
    # four event reals (adjusted Rand index, purity, efficiency, mutual fraction).  '' = off.  Refused without ANA_CLUSTER; ignored
    # with TRAIN, like every ANA_* key
    ANA_MATCH = ''
    # ANA_GRAPH '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per interaction group: the connected components of the
    # predicted clusters under "some voxel of one lies within GRAPH_GAP voxels of some voxel of the other on every axis"
    # (ssnet_base.set_cluster_graph; clusters.cluster_graph_numpy holds the definition): entry, group and the twelve group integers
    # (rows, edges, entries, fixed-point charge, box, first row, class mask | flags << 32).  '' = off.  Refused without ANA_CLUSTER;
    # ignored with TRAIN, like every ANA_* key.  GRAPH_GAP = 1, 2 or 3
    ANA_GRAPH = ''
    GRAPH_GAP = 1
    # ANA_PROFILES '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per cluster: the row record of its charge profile along
    # the principal axis (ssnet_base.set_cluster_profiles; clusters.cluster_profile_numpy holds the definition): entry, id, the
    # twelve row integers (bins, filled, gaps, longest gap, peak bin, end bins, count and fixed-point charge at the head and the
    # tail, the sign of their charge asymmetry, flags) and the six row reals (path, smallest cosine, its bin, dQ/dx at the head and
    # the tail, straightness).  '' = off.  Refused without ANA_CLUSTER; ignored with TRAIN, like every ANA_* key.  PROFILE_STEP =
    # the segment length in voxels, a float in [0.5, 4096]; PROFILE_END_BINS = 1 .. 16 segments at either end
    ANA_PROFILES = ''
    PROFILE_STEP = 1.0
    PROFILE_END_BINS = 3
    # ANA_VERTICES '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per vertex candidate: a point where end points of the
    # clusters' object records meet within VERTEX_RADIUS voxels (ssnet_base.set_cluster_vertices; clusters.cluster_vertices_numpy
    # holds the definition): entry, vertex, the seventeen vertex integers (ends, incident rows, bodies passing by, near entries,
    # entries and fixed-point charge of the incident rows, sum and box of the end-point coordinates, first end position, class mask
    # | flags << 32) and the five reals (centroid, smallest and largest cosine between the end directions).  '' = off.  Refused
    # without ANA_CLUSTER; ignored with TRAIN, like every ANA_* key.  VERTEX_RADIUS = 1, 2 or 3; VERTEX_MIN_SIZE = smaller clusters
    # have no end points; VERTEX_CLASSES = the classes whose clusters have end points, [] = all
    ANA_VERTICES = ''
    VERTEX_RADIUS = 2
    VERTEX_MIN_SIZE = 3
    VERTEX_CLASSES = []
    # ANA_CHAINS '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per chain: clusters that are fragments of one broken track,
    # joined end to end across gaps of at most CHAIN_GAP voxels per axis when both axes and the gap vector are collinear within
    # CHAIN_MIN_COS and the choice is mutual (ssnet_base.set_cluster_chains; clusters.cluster_chains_numpy holds the definition):
    # entry, chain, the sixteen chain integers (rows, joins, entries, fixed-point charge, box, first row, the two end positions,
    # sum and maximum of the squared gaps, class mask | flags << 32) and the five reals (path, gaps, span, straightness, smallest
    # cosine between joined axes).  '' = off.  Refused without ANA_CLUSTER; ignored with TRAIN, like every ANA_* key.  CHAIN_GAP =
    # 1 .. 31; CHAIN_MIN_COS = a float in [0, 1]; CHAIN_MIN_SIZE = smaller clusters are not joined; CHAIN_CLASSES = the classes whose
    # clusters are joined, [] = all; CHAIN_SAME_CLASS = only clusters of equal class are joined
    ANA_CHAINS = ''
    CHAIN_GAP = 6
    CHAIN_MIN_COS = 0.9
    CHAIN_MIN_SIZE = 3
    CHAIN_CLASSES = []
    CHAIN_SAME_CLASS = True
    # ANA_CONES '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per shower: clusters that are fragments of one
    # electromagnetic shower, each linked to the nearest end point of a larger cluster within CONE_REACH voxels inside whose cone
    # of cosine CONE_MIN_COS it lies (ssnet_base.set_cluster_cones; clusters.cluster_cones_numpy holds the definition): entry,
    # shower, the sixteen shower integers (rows, entries, fixed-point charge, box, first row, primary, start position, depth,
    # largest squared distance, entries of the primary, class mask | flags << 32) and the four reals (primary fraction, smallest
    # cone cosine, largest axial distance, largest distance).  '' = off.  Refused without ANA_CLUSTER; ignored with TRAIN, like
    # every ANA_* key.  CONE_REACH = 1 .. 127; CONE_MIN_COS = a float in (0, 1]; CONE_SEED_SIZE = smaller clusters are no parent
    # (>= 2); CONE_MIN_SIZE = smaller clusters are no child; CONE_CLASSES = the classes whose clusters take part, [] = all;
    # CONE_SAME_CLASS = only clusters of equal class are linked
    ANA_CONES = ''
    CONE_REACH = 48
    CONE_MIN_COS = 0.8
    CONE_SEED_SIZE = 8
    CONE_MIN_SIZE = 1
    CONE_CLASSES = []
    CONE_SAME_CLASS = True
    # ANA_SPLIT '<file>' (with TRAIN False and ANA_CLUSTER) = one CSV row per junction: the places where a cluster that holds several
    # particles is cut -- voxels that see three or more arms inside a ball of SPLIT_RADIUS, or two arms whose cosine exceeds
    # SPLIT_KINK_COS (ssnet_base.set_cluster_split; clusters.cluster_split_numpy holds the definition): entry, junction, the
    # eighteen junction integers (row, entries, attached, largest arm count, kink entries, coordinate sums, box, first position,
    # contacts, lowest and highest piece it touches) and the centroid.  '' = off.  Refused without ANA_CLUSTER; ignored with TRAIN,
    # like every ANA_* key.  SPLIT_RADIUS = 1 .. 3; SPLIT_KINK_COS = a float in [-1, 1], 1 = no kinks; SPLIT_MIN_SIZE = smaller
    # clusters stay whole; SPLIT_CLASSES = the classes whose clusters are split, [] = all; SPLIT_GROW = 0 .. 8 attachment rounds,
    # -1 = twice the radius; SPLIT_DOWNSTREAM = the object, profile, vertex, chain, cone and graph records describe the pieces
    ANA_SPLIT = ''
    SPLIT_RADIUS = 2
    SPLIT_KINK_COS = -0.7
    SPLIT_MIN_SIZE = 8
    SPLIT_CLASSES = []
    SPLIT_GROW = -1
    SPLIT_DOWNSTREAM = False

    def __init__(self):
        pass

    @classmethod
    def _keys(cls):
        return [s for s in ssnet_config.__dict__.keys() if s == s.upper() and not s.startswith('_')]

    def override(self, file_name):
        """lib/config.py:40-66.  Raises IOError for a missing file and TypeError for a value whose
        type differs from the default's (LEARNING_RATE excepted, lib/config.py:62)."""
        keys = self._keys()
        if not os.path.isfile(file_name):
            print('Config file not found', file_name)
            raise IOError(file_name)
        with open(file_name, 'r') as f:
            lines = f.read().split('\n')
        for line in lines:
            valid_line = line
            if line.find('#') >= 0:
                valid_line = line[0:line.find('#')]
            words = valid_line.split(None, 1)
            if len(words) == 0:
                continue
            if len(words) != 2:
                print('Ignoring a line:', line)
                continue
            key, text = words[0], words[1].strip()
            if key not in keys:
                print('Ignoring a parameter in file:', key)
                continue
            try:
                value = ast.literal_eval(text)
            except (ValueError, SyntaxError):
                print('Incompatible type: %s' % line)
                raise TypeError(line)
            if key != 'LEARNING_RATE' and type(getattr(self, key)) != type(value):
                print('Incompatible type: %s' % line)
                raise TypeError(line)
            if key == 'PRECISION' and value not in ('fp32', 'bf16'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'AUGMENT' and value not in ('', 'flip', 'cube'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'ANA_BN' and value not in ('batch', 'moving'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'TRAIN_BN' and value not in ('batch', 'frozen'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'BN_DECAY' and not 0.0 <= value <= 1.0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'DEVICE_WEIGHTS' and value not in ('', 'class', 'invfreq'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'WEIGHT_RADIUS' and not 0 <= value <= 3:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'WEIGHT_SCALE' and not all(type(c) in (int, float) and c == c and abs(c) != float('inf') for c in value):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key in ('CLIP_GRAD_NORM', 'WEIGHT_DECAY') and not 0.0 <= value < float('inf'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key in ('LR_WARMUP_STEPS', 'LR_DECAY_STEPS') and value < 0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'LR_DECAY_RATE' and not 0.0 < value < float('inf'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'ANA_TTA' and not all(type(c) is int and 0 <= c < 48 for c in value):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key in ('ANA_TILE', 'TRAIN_CROP') and not (len(value) in (0, 2, 3) and all(type(c) is int and c >= 1 for c in value)):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'ANA_TILE_HALO' and value < 0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'ANA_TILE_BATCH' and value < 1:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'LOSS_FOCAL_GAMMA' and not (value == 0.0 or 1.0 <= value < float('inf')):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'LOSS_LABEL_SMOOTHING' and not 0.0 <= value < 1.0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'LOSS_DICE_WEIGHT' and not 0.0 <= value < float('inf'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'LOSS_DICE_EPS' and not 0.0 < value < float('inf'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'ANA_CLUSTER' and value not in ('', 'pred', 'ana'):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CLUSTER_CONNECTIVITY' and value not in (0, 4, 8, 6, 18, 26):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CLUSTER_CLASSES' and not (all(type(c) is int and 0 <= c < 32 for c in value)
                                                 and len(set(value)) == len(value)):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CLUSTER_MIN_SIZE' and value < 1:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'GRAPH_GAP' and not 1 <= value <= 3:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'VERTEX_RADIUS' and not 1 <= value <= 3:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'VERTEX_MIN_SIZE' and value < 1:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'VERTEX_CLASSES' and not (all(type(c) is int and 0 <= c < 32 for c in value) and len(set(value)) == len(value)):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'SPLIT_RADIUS' and not 1 <= value <= 3:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'SPLIT_KINK_COS' and not -1.0 <= value <= 1.0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'SPLIT_MIN_SIZE' and value < 1:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'SPLIT_GROW' and not -1 <= value <= 8:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'SPLIT_CLASSES' and not (all(type(c) is int and 0 <= c < 32 for c in value) and len(set(value)) == len(value)):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CHAIN_GAP' and not 1 <= value <= 31:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CHAIN_MIN_COS' and not 0.0 <= value <= 1.0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CHAIN_MIN_SIZE' and value < 1:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CHAIN_CLASSES' and not (all(type(c) is int and 0 <= c < 32 for c in value) and len(set(value)) == len(value)):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CONE_REACH' and not 1 <= value <= 127:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CONE_MIN_COS' and not 0.0 < value <= 1.0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CONE_SEED_SIZE' and value < 2:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CONE_MIN_SIZE' and value < 1:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'CONE_CLASSES' and not (all(type(c) is int and 0 <= c < 32 for c in value) and len(set(value)) == len(value)):
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'PROFILE_STEP' and not 0.5 <= value <= 4096.0:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            if key == 'PROFILE_END_BINS' and not 1 <= value <= 16:
                print('Incompatible value: %s' % line)
                raise TypeError(line)
            setattr(self, key, value)

    def cluster_spec(self):
        """The clusters.ClusterSpec of the CLUSTER_* keys, or None while ANA_CLUSTER is off."""
        if not self.ANA_CLUSTER:
            return None
        from .clusters import ClusterSpec
        return ClusterSpec(self.CLUSTER_CONNECTIVITY or None, self.CLUSTER_CLASSES or None, True, self.CLUSTER_MIN_SIZE,
                           self.ANA_CLUSTER)

    def loss_spec(self):
        """The losses.LossSpec of the LOSS_* keys, or None while they all hold their defaults (the plan's head runs)."""
        from .losses import LossSpec
        spec = LossSpec(self.LOSS_FOCAL_GAMMA, self.LOSS_LABEL_SMOOTHING, self.LOSS_DICE_WEIGHT, self.LOSS_DICE_EPS,
                        self.LOSS_IGNORE_LABEL)
        return None if spec.neutral else spec

    def dump(self):
        """lib/config.py:68-76."""
        for key in self._keys():
            msg = key
            while len(msg) < 20:
                msg += '.'
            print('%s %s' % (msg, str(getattr(self, key))))


if __name__ == '__main__':
    import sys
    k = ssnet_config()
    k.dump()
    if len(sys.argv) > 1:
        k.override(sys.argv[1])
        print('\n')
        k.dump()

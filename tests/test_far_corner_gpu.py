"""The front end's stand-alone calls in the largest volume: cluster_voxels -> cluster_split -> cluster_chains ->
cluster_cones, and the object records, profiles, vertices and the graph of the pieces, with shape = (2047, 1024, 1024) on the
translated random events of tests/_far_corner.py, each against the same chain of statements through the comparison helpers of the
calls' own modules.  This is what catches a wrapper that sizes anything by prod(shape) or narrows an index on the way in or out;
the op-level far-corner tests live in the modules of the calls."""
import numpy as np
import pytest

import _far_corner as far
from test_cluster_chain_gpu import _same_chains
from test_cluster_cone_gpu import _same_cones
from test_cluster_features_gpu import _same_objects
from test_cluster_graph_gpu import _same_graph, _toff
from test_cluster_profile_gpu import _same_profiles
from test_cluster_split_gpu import _same_split
from test_cluster_vertex_gpu import _same_vertices
from test_clusters_gpu import _same_clusters
from uresnet_amd import uresnet
from uresnet_amd.clusters import (ClusterChainSpec, ClusterConeSpec, ClusterGraphSpec, ClusterProfileSpec, ClusterSplitSpec,
                                  ClusterVertexSpec, cluster_graph_numpy)
from uresnet_amd.ssnet import VoxelBatch

pytestmark = pytest.mark.gpu


def test_the_front_end_in_the_largest_volume():
    shape = far.LARGEST_VOLUME
    fb = far.far_batch("random", shape)
    b = fb.big
    n = b.off.size - 1
    assert set(fb.placement) == {far.FAR, far.ORIGIN, far.MIDDLE, None} and int(b.index.max()) > 2 ** 31 - 2 ** 21
    vb = VoxelBatch(b.off, b.index.astype(np.int32), b.value, voxels=far.volume(shape)).validate()
    lists = [vb.index[b.off[e]:b.off[e + 1]] for e in range(n)]
    classes = [b.cls[b.off[e]:b.off[e + 1]] for e in range(n)]
    net = uresnet(dims=[16, 16, 16, 1], num_class=3, base_num_outputs=4, num_strides=2)      # the calls take their shape as an argument
    net.construct(trainable=False, use_weight=False, seed=7, precision="fp32")
    made = net.cluster_voxels(None, vb, classes, far.SPEC_3D, shape=shape)
    _same_clusters(dict(made, index=lists), classes, shape, far.SPEC_3D)
    assert np.array_equal(np.concatenate(made["cluster"]), b.cluster)
    # the split of those clusters, then everything downstream on the pieces
    split_spec = ClusterSplitSpec(2, -0.7, 4)
    pieces = net.cluster_split(None, vb, made, split_spec, shape=shape)
    want = _same_split(pieces, vb, b.index, made, shape, split_spec)
    assert want["piece_offsets"][-1] > b.toff[-1]                                            # something was split
    r = dict(index=lists, cluster=pieces["cluster"], clusters=pieces["clusters"])
    chain_spec = ClusterChainSpec(31, 0.7, 2, None, False)
    chains = net.cluster_chains(None, vb, None, pieces, chain_spec, shape=shape)
    assert _same_chains(r, vb, shape, chain_spec, got=chains)["join_offsets"][-1] > 0
    cone_spec = ClusterConeSpec(127, 0.7, 4, 1, None, False)
    cones = net.cluster_cones(None, vb, None, chains, cone_spec, shape=shape)
    assert _same_cones(chains, lists, vb, shape, cone_spec, cones)["link_offsets"][-1] > 0
    _same_objects(dict(r, objects=net.cluster_features(None, vb, None, pieces, shape=shape)), vb, shape)
    profile_spec = ClusterProfileSpec(0.5, 16, 65536)
    _same_profiles(dict(r, profiles=net.cluster_profiles(None, vb, None, pieces, profile_spec, shape=shape)), vb, shape, profile_spec)
    vertex_spec = ClusterVertexSpec(3, 2)
    _same_vertices(dict(r, vertices=net.cluster_vertices(None, vb, None, pieces, vertex_spec, shape=shape)), vb, shape, vertex_spec)
    toff = _toff(pieces["clusters"])
    graph = cluster_graph_numpy(vb.offsets, b.index, np.concatenate(pieces["cluster"]), toff, shape, ClusterGraphSpec(3), vb.value,
                                np.concatenate([t["cls"] for t in pieces["clusters"]]))
    _same_graph(net.cluster_graph(None, vb, pieces, ClusterGraphSpec(3), shape=shape), graph, vb.offsets, toff)
    assert graph["edge_offsets"][-1] > 0

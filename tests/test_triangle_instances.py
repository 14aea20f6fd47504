"""The frame table's eligibility rule on the host (dcrt_flat_scene_triangle_instances, bvh_layout.cpp's
TriangleInstances): the instance of every triangle where each BLAS has one instance; refused where a
BLAS has two, or where the tree is malformed."""
import numpy as np

import random_scenes as RS
from conftest import cornell
from directcomputeraytracing_amd import _abi
from directcomputeraytracing_amd.scene import flat_triangle_instances

NONE = 0xFFFFFFFF


def _nodes(flat):
    return (_abi.BVHNode * flat.bvh_node_count)(*[flat.bvh_nodes[i] for i in range(flat.bvh_node_count)])


def _tlas_leaves(flat):
    return [i for i in range(flat.tlas_node_count) if flat.bvh_nodes[i].misc & 4]


def test_cornell_every_blas_has_one_instance(native_lib):
    scene = cornell(32, 32, 2)
    single, owners = scene.triangle_instances()
    flat = scene.flat()
    assert single and len(owners) == flat.triangle_count == 32 and flat.instance_count == 8
    assert (owners < 8).all() and sorted(set(owners.tolist())) == list(range(8))
    # (a BLAS leaf's triangles are consecutive: every instance owns whole runs of the triangle array)
    assert (np.diff(owners) != 0).sum() == 7


def test_a_mesh_instanced_twice_is_refused(native_lib, tmp_path):
    from directcomputeraytracing_amd import Scene
    scene = Scene((32, 24))
    scene.load_from_file(RS.write_xml_scene(tmp_path, 5, 32, 24, n_grid=2, n_loose=2, n_instances=2))
    assert scene.flat().instance_count == 4
    assert scene.triangle_instances()[0] is False


def test_two_tlas_leaves_on_one_blas_are_refused(native_lib):
    scene = cornell(32, 32, 2)
    flat = scene.flat()
    nodes = _nodes(flat)
    a, b = _tlas_leaves(flat)[:2]
    nodes[b].right_child_or_prim_index = nodes[a].right_child_or_prim_index
    flat.bvh_nodes = nodes
    assert flat_triangle_instances(native_lib, flat)[0] is False


def test_triangles_no_instance_reaches_have_no_owner(native_lib):
    scene = cornell(32, 32, 2)
    flat = scene.flat()
    _, whole = flat_triangle_instances(native_lib, flat)
    nodes = _nodes(flat)
    leaf = _tlas_leaves(flat)[0]
    inst = nodes[leaf].misc >> 3
    nodes[0] = nodes[leaf]                 # the TLAS is this one leaf
    flat.bvh_nodes = nodes
    single, owners = flat_triangle_instances(native_lib, flat)
    assert single
    assert ((owners == inst) == (whole == inst)).all() and (owners[whole != inst] == NONE).all() and (owners == inst).any()


def test_malformed_trees_are_refused(native_lib):
    scene = cornell(32, 32, 2)
    for what in ("child out of range", "triangle out of range", "instance out of range"):
        flat = scene.flat()
        nodes = _nodes(flat)
        leaf = _tlas_leaves(flat)[0]
        if what == "child out of range":
            nodes[leaf].right_child_or_prim_index = flat.bvh_node_count + 5
        elif what == "instance out of range":
            nodes[leaf].misc = (flat.instance_count << 3) | 4
        else:
            blas = next(i for i in range(flat.tlas_node_count, flat.bvh_node_count) if nodes[i].misc >= 4)
            nodes[blas].right_child_or_prim_index = flat.triangle_count
        flat.bvh_nodes = nodes
        assert flat_triangle_instances(native_lib, flat)[0] is False, what
    assert native_lib.dcrt_flat_scene_triangle_instances(None, None, 0, None) != 0

"""Hand-built BVH shapes over the triangles of a loaded scene. Test infrastructure only.

include/rrt.h lets a caller fill the scene description, and validate_desc (host/scene_flatten.cpp) checks the links, the pre-order and the depth bound of a
caller's tree before anything reaches a device - so a hand-built tree is legitimate input, and the only way to walk the traversal kernels through
tree shapes the project's own builder never makes: chains deeper than the 8-entry LDS stacks and than the 64-entry private stack, a root that is a
leaf, leaves at the limits of the pair-node and quad-node leaf words.

A shape is a copy of the scene's description (SceneDesc.from_buffer_copy) that points at its own rrt_bvh_node array and prim_order; everything else
stays the scene's, which the shape keeps alive. It has .desc and .resolution, all that Renderer and oracle_lib read. RRT_FIXED_BVH is set in its
flags: it is what tells the oracle that the tree is not the reference builder's, i.e. that the reference's nodes_to_visit[64] does not apply (the
device does not read the bit).

Every shape is built for an exact bvh_depth (root = 1, as the host builder and validate_desc count); .depth is measured from the finished array.
Per-primitive bounds come from the vertex positions in f64, padded by 1e-9 of the largest coordinate; interior boxes are exact unions; the layout is
flattern_bvh's pre-order (first child at i + 1, second child after the first child's whole subtree).
"""
import ctypes as C

import numpy as np

from rs_ray_toy_amd import RRT_FIXED_BVH
from rs_ray_toy_amd import _abi as A


def prim_bounds(scene):
    """(n_prims, 6) f64 boxes {min xyz, max xyz} of the scene's primitives, which must be plain un-instanced triangles."""
    d = scene.desc
    n = d.n_prims
    prims = np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(C.c_uint8)), (n, C.sizeof(A.Prim))).view(
        np.dtype({"names": ["type", "shape", "instance"], "formats": ["u1", "<u4", "<i4"], "offsets": [A.Prim.type.offset, A.Prim.shape.offset, A.Prim.instance.offset],
                  "itemsize": C.sizeof(A.Prim)})).reshape(n)
    assert np.all(prims["type"] == A.RRT_PRIM_TRIANGLE) and np.all(prims["instance"] < 0), "shapes are built over plain, un-instanced triangles"
    tris = np.ctypeslib.as_array(C.cast(d.tris, C.POINTER(C.c_uint32)), (d.n_tris, C.sizeof(A.Tri) // 4))[:, :3]
    pos = np.ctypeslib.as_array(d.positions, (d.n_positions, 3))
    p = pos[tris[prims["shape"]]]                      # (n, 3 vertices, 3)
    pad = 1e-9 * np.abs(pos).max()
    return np.concatenate([p.min(1) - pad, p.max(1) + pad], 1)


def shortest_edge(scene):
    d = scene.desc
    tris = np.ctypeslib.as_array(C.cast(d.tris, C.POINTER(C.c_uint32)), (d.n_tris, C.sizeof(A.Tri) // 4))[:, :3]
    p = np.ctypeslib.as_array(d.positions, (d.n_positions, 3))[tris]
    return min(float(np.linalg.norm(p[:, a] - p[:, b], axis=1).min()) for a, b in ((0, 1), (1, 2), (2, 0)))


# ---- tree descriptions: ("leaf", [prim, ...]) or ("node", axis, first, second) ----------------------------------------------------------------
def _balanced(ids, bounds, leaf_max):
    """Median split along the longest axis of the centroid bounds, down to leaves of at most leaf_max primitives."""
    ids = np.asarray(ids)
    if len(ids) <= leaf_max:
        return ("leaf", [int(i) for i in ids])
    c = (bounds[ids, :3] + bounds[ids, 3:]) * 0.5
    axis = int(np.argmax(c.max(0) - c.min(0)))
    ids = ids[np.argsort(c[:, axis], kind="stable")]
    h = (len(ids) + 1) // 2
    return ("node", axis, _balanced(ids[:h], bounds, leaf_max), _balanced(ids[h:], bounds, leaf_max))


def _balanced_depth(n, leaf_max):
    return 1 if n <= leaf_max else 1 + _balanced_depth((n + 1) // 2, leaf_max)


def _chain(groups, tail, side):
    """groups[0] is the root's leaf child, tail the subtree below the last interior node. side: "first" / "second" / "alt" = where the leaf child goes.
    The split axis field cycles 0 / 1 / 2 down the chain: it only orders the two children's visits."""
    tree = tail
    for level in range(len(groups) - 1, -1, -1):
        leaf = ("leaf", [int(i) for i in groups[level]])
        first = side == "first" or (side == "alt" and level % 2 == 0)
        tree = ("node", level % 3, leaf, tree) if first else ("node", level % 3, tree, leaf)
    return tree


def _flatten(tree, bounds):
    """-> (nodes: list of [box6, offset, n_primitives, axis], order: list of prim ids, depth), iteratively (chains are hundreds of levels deep)."""
    nodes, order = [], []
    depth = 0
    # pre-order emission with an explicit stack; an interior node's offset and box are patched once its children are known
    todo = [("visit", tree, 1, None)]
    while todo:
        what, t, lvl, parent = todo.pop()
        if what == "visit":
            depth = max(depth, lvl)
            me = len(nodes)
            if parent is not None and parent[1] == "second":
                nodes[parent[0]][1] = me
            if t[0] == "leaf":
                ids = t[1]
                assert len(ids) > 0
                b = bounds[ids]
                nodes.append([np.concatenate([b[:, :3].min(0), b[:, 3:].max(0)]), len(order), len(ids), 0])
                order.extend(ids)
            else:
                nodes.append([None, 0, 0, t[1]])
                todo.append(("close", me, lvl, None))
                todo.append(("visit", t[3], lvl + 1, (me, "second")))
                todo.append(("visit", t[2], lvl + 1, (me, "first")))
        else:
            me = t
            a, b = nodes[me + 1][0], nodes[nodes[me][1]][0]
            nodes[me][0] = np.concatenate([np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])])
    return nodes, order, depth


class ShapedScene:
    """A scene description with a hand-built tree: .desc, .resolution, .depth (= desc.bvh_depth), .leaf_sizes, .name."""

    def __init__(self, scene, tree, name, bounds=None):
        bounds = prim_bounds(scene) if bounds is None else bounds
        nodes, order, depth = _flatten(tree, bounds)
        assert sorted(order) == list(range(scene.desc.n_prims)), "every primitive exactly once"
        self.base, self.name, self.depth = scene, name, depth
        self.axis = None      # chain / comb: the axis the primitives were sorted along
        self.leaf_sizes = [n[2] for n in nodes if n[2] > 0]
        self.n_interior = sum(1 for n in nodes if n[2] == 0)
        self._nodes = (A.BvhNode * len(nodes))()
        for dst, (box, offset, n_prims, axis) in zip(self._nodes, nodes):
            dst.bounds[:] = [float(x) for x in box]
            dst.offset, dst.n_primitives, dst.axis, dst.pad = offset, n_prims, axis, 0
        self._order = (C.c_uint32 * len(order))(*order)
        self.desc = A.SceneDesc.from_buffer_copy(scene.desc)
        self.desc.bvh_nodes = C.cast(self._nodes, C.POINTER(A.BvhNode))
        self.desc.n_bvh_nodes = len(nodes)
        self.desc.prim_order = C.cast(self._order, C.POINTER(C.c_uint32))
        self.desc.n_prim_order = len(order)
        self.desc.bvh_depth = depth
        self.desc.flags |= RRT_FIXED_BVH
        self.last_interior_box = next(np.array(n[0]) for n in reversed(nodes) if n[2] == 0) if self.n_interior else np.array(nodes[0][0])

    @property
    def resolution(self):
        return self.desc.film.xres, self.desc.film.yres


def _sorted_ids(bounds, sort_axis):
    return np.argsort((bounds[:, sort_axis] + bounds[:, 3 + sort_axis]) * 0.5, kind="stable")


def chain(scene, depth, side="first", sort_axis=0):
    """A caterpillar of exactly `depth` levels: depth - 1 interior nodes, each with one leaf of k primitives and "the rest"; the last rest is a leaf."""
    bounds = prim_bounds(scene)
    ids = _sorted_ids(bounds, sort_axis)
    n = len(ids)
    if depth == 1:
        return one_leaf(scene)
    assert 2 <= depth <= n
    k = n // depth
    groups = [ids[i * k:(i + 1) * k] for i in range(depth - 1)]
    sh = ShapedScene(scene, _chain(groups, ("leaf", [int(i) for i in ids[(depth - 1) * k:]]), side), f"chain_{side}_{depth}", bounds)
    assert sh.depth == depth, (sh.depth, depth)
    sh.axis = sort_axis
    return sh


def comb(scene, depth, side="alt", sort_axis=2, k=1):
    """A chain whose last group is a median-split balanced subtree: `depth` levels in all, the chain as long as that allows."""
    bounds = prim_bounds(scene)
    ids = _sorted_ids(bounds, sort_axis)
    n = len(ids)
    for leaf_max in (1, 2, 4, 8, 16, 32, 64):      # small leaves first: the most interior nodes (the tile-tree census wants more than its copy holds)
        for c in range(min(depth - 1, (n - 1) // k), 0, -1):      # c chain levels, then the balanced subtree
            if c + _balanced_depth(n - c * k, leaf_max) == depth:
                groups = [ids[i * k:(i + 1) * k] for i in range(c)]
                sh = ShapedScene(scene, _chain(groups, _balanced(ids[c * k:], bounds, leaf_max), side), f"comb_{side}_{depth}", bounds)
                assert sh.depth == depth, (sh.depth, depth)
                sh.axis = sort_axis
                return sh
    raise ValueError(f"no comb of depth {depth} over {n} primitives")


def one_leaf(scene):
    """The root is a leaf that holds every primitive."""
    sh = ShapedScene(scene, ("leaf", list(range(scene.desc.n_prims))), "one_leaf")
    assert sh.depth == 1 and sh.n_interior == 0
    return sh


def fat(scene, big, leaf_max=320, sort_axis=0):
    """A small balanced tree beside one leaf of exactly `big` primitives (the first `big` along sort_axis); every other leaf holds at most leaf_max."""
    bounds = prim_bounds(scene)
    ids = _sorted_ids(bounds, sort_axis)
    assert 0 < big < len(ids) and leaf_max < big
    sh = ShapedScene(scene, ("node", sort_axis, ("leaf", [int(i) for i in ids[:big]]), _balanced(ids[big:], bounds, leaf_max)), f"fat_{big}", bounds)
    assert max(sh.leaf_sizes) == big and sorted(sh.leaf_sizes)[-2] <= leaf_max
    return sh

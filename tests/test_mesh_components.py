"""Mesh connected components and floater removal (cnr_mesh_components / cnr_mesh_select / cnr_mesh_compact; color_neus_amd.meshops,
NeuSRenderer.extract_geometry / render_mesh_view with ``clean=``).

The yardstick is a sequential union-find written here (``_yardstick``: min-index roots, the same validity rule) and, for selection and
compaction, numpy boolean indexing.  Everything is integer work or a copy, so EVERY comparison is exact: integer for integer, and float
payloads bit for bit.  Every case runs on the CPU emulation build and (``-m gpu``) on the HIP build; the two are compared with the same
yardstick, hence with each other."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import color_neus_amd as cn
from color_neus_amd import _lib, meshops
import _golden as G
import _guard
import _native as N

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
# cnr_meshcc.h: kMeshScanChunk = kMeshScanThreads * kMeshScanPer = 1024 * 8, the elements one trip of the single-workgroup carried scan
# (meshcc_scan_kernel, cnr_meshcc.hip) takes in; the other kernels work in workgroups of 256 lanes = 4 waves of 64
SCAN_CHUNK = 8192
EDGE_SIZES = [1, 63, 64, 65, 255, 256, 257, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1]
LARGEST, THRESHOLD = 0, 1


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return cn.load_library(N.EMU_LIB), "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return cn.load_library(), "cuda:0"


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def _yardstick(tris, V):
    """labels, face_count, vertex_count (int32 [V]), summary [4], dropped of the definitions in include/colorneus_render.h, sequentially."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    parent = list(range(V))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    valid = ((tris >= 0) & (tris < V)).all(axis=1) if len(tris) else np.zeros(0, bool)
    for a, b, c in tris[valid].tolist():
        for x in (b, c):
            ra, rx = find(a), find(x)
            if ra != rx:
                parent[max(ra, rx)] = min(ra, rx)
    labels = np.array([find(v) for v in range(V)], np.int32).reshape(V)
    face_count, vertex_count = np.zeros(V, np.int32), np.zeros(V, np.int32)
    np.add.at(vertex_count, labels, 1)
    if valid.any():
        np.add.at(face_count, labels[tris[valid][:, 0]], 1)
    roots = np.nonzero(labels == np.arange(V))[0]
    with_faces = roots[face_count[roots] > 0]
    if len(with_faces):
        best = with_faces[np.argmax(face_count[with_faces])]        # argmax: the first = the lowest label of equal counts
        summary = [len(roots), len(with_faces), int(best), int(face_count[best])]
    else:
        summary = [len(roots), 0, -1, 0]
    return {"labels": labels, "face_count": face_count, "vertex_count": vertex_count, "summary": np.array(summary, np.int32),
            "dropped": int((~valid).sum()), "valid": valid}


def _yard_select(tris, V, y, mode, min_faces=0, min_ratio=0.0):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    largest_label, largest = int(y["summary"][2]), int(y["summary"][3])
    thr = max(int(min_faces), int(np.ceil(np.float32(min_ratio) * np.float32(largest))))
    comp_faces = y["face_count"][y["labels"]] if V else np.zeros(0, np.int32)       # per vertex: the faces of its component
    comp_kept = (y["labels"] == largest_label) if mode == LARGEST else (comp_faces >= thr)
    keep_vertex = comp_kept & (comp_faces > 0)
    keep_face = np.zeros(len(tris), bool)
    keep_face[y["valid"]] = comp_kept[tris[y["valid"]][:, 0]]
    vertex_map = np.where(keep_vertex, np.cumsum(keep_vertex) - 1, -1).astype(np.int32)
    face_map = np.where(keep_face, np.cumsum(keep_face) - 1, -1).astype(np.int32)
    return {"keep_vertex": keep_vertex.astype(np.uint8), "keep_face": keep_face.astype(np.uint8), "vertex_map": vertex_map, "face_map": face_map,
            "totals": np.array([keep_vertex.sum(), keep_face.sum()], np.int32)}


# ---- the three entries on caller-owned typed buffers ------------------------------------------------------------------------------------------
OUT_KEYS = ("labels", "face_count", "vertex_count", "summary", "dropped", "keep_vertex", "keep_face", "vertex_map", "face_map", "totals",
            "out_vertices", "out_colors", "out_triangles")


def _raw(lib, dev, tris, V, verts=None, cols=None, mode=LARGEST, min_faces=0, min_ratio=0.0, guard=None):
    """cnr_mesh_components -> cnr_mesh_select -> (with verts) cnr_mesh_compact; every output an exact-size typed buffer (from ``guard`` if
    given: poisoned payloads between guard bytes, the inputs copied between NaN guards).  Returns numpy arrays by name."""
    tris = torch.as_tensor(np.ascontiguousarray(np.asarray(tris, np.int32).reshape(-1, 3))).to(dev)
    F = tris.shape[0]
    if guard is None:
        bases = []

        def empty(shape, dt):        # (an empty tensor has no address of its own: the zero-length head of a one-row allocation has one)
            shape = shape if isinstance(shape, tuple) else (shape,)
            base = torch.empty((max(shape[0], 1),) + shape[1:], dtype=dt, device=dev)
            bases.append((base[:shape[0]], base))
            return bases[-1][0]

        def addr(t):
            return _lib.ptr(next((base for view, base in bases if view is t), t))

        def inp(t):
            if t.numel() == 0:
                bases.append((t, torch.empty((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)))
            return t
    else:
        empty = lambda shape, dt: guard.empty(shape, dt, dev)
        addr, inp = guard.addr, guard.copy
    t = inp(tris)
    i32, u8, f32 = torch.int32, torch.uint8, torch.float32
    o = {"labels": empty(V, i32), "face_count": empty(V, i32), "vertex_count": empty(V, i32), "summary": empty(4, i32), "dropped": empty(1, i32),
         "keep_vertex": empty(V, u8), "keep_face": empty(F, u8), "vertex_map": empty(V, i32), "face_map": empty(F, i32), "totals": empty(2, i32)}
    stream = _lib.stream_of(torch.device(dev))
    lib.call("cnr_mesh_components", addr(t), F, V, addr(o["labels"]), addr(o["face_count"]), addr(o["vertex_count"]), addr(o["summary"]),
             addr(o["dropped"]), stream)
    lib.call("cnr_mesh_select", addr(t), F, V, addr(o["labels"]), addr(o["face_count"]), addr(o["summary"]), mode, int(min_faces), float(min_ratio),
             addr(o["keep_vertex"]), addr(o["keep_face"]), addr(o["vertex_map"]), addr(o["face_map"]), addr(o["totals"]), stream)
    if verts is not None:
        nv, nf = (int(x) for x in o["totals"].tolist())
        v = inp(torch.as_tensor(np.asarray(verts, np.float32).reshape(V, 3)).to(dev))
        c = inp(torch.as_tensor(np.asarray(cols, np.float32).reshape(V, 3)).to(dev)) if cols is not None else None
        o["out_vertices"], o["out_triangles"] = empty((nv, 3), f32), empty((nf, 3), i32)
        o["out_colors"] = empty((nv, 3), f32) if cols is not None else None
        null = C.c_void_p(0)
        lib.call("cnr_mesh_compact", addr(v), addr(c) if c is not None else null, addr(t), F, V, addr(o["vertex_map"]), addr(o["face_map"]),
                 addr(o["out_vertices"]), addr(o["out_colors"]) if c is not None else null, addr(o["out_triangles"]), stream)
    if guard is not None:
        guard.check()
    return {k: (x.cpu().numpy().copy() if x is not None else None) for k, x in o.items()}


def _check_components(got, y):
    for k in ("labels", "face_count", "vertex_count", "summary"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], y[k]), k
    assert int(got["dropped"][0]) == y["dropped"]


def _check_select(got, want):
    for k in ("keep_vertex", "keep_face", "vertex_map", "face_map", "totals"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def _check_compact(got, tris, verts, cols, sel):
    """vertices' = vertices[keep], colours likewise, to the bit and in the original order; triangles' = vertex_map[triangles[keep_face]]."""
    kv, kf = sel["keep_vertex"].astype(bool), sel["keep_face"].astype(bool)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    assert np.array_equal(got["out_vertices"].view(np.int32), np.asarray(verts, np.float32)[kv].view(np.int32))
    if cols is not None:
        assert np.array_equal(got["out_colors"].view(np.int32), np.asarray(cols, np.float32)[kv].view(np.int32))
    want = sel["vertex_map"][tris[kf]] if kf.any() else np.zeros((0, 3), np.int32)
    assert np.array_equal(got["out_triangles"], want)
    if len(want):
        assert got["out_triangles"].min() >= 0 and got["out_triangles"].max() < kv.sum()


def _full(lib, dev, tris, V, mode=LARGEST, min_faces=0, min_ratio=0.0, seed=0, colors=True, guard=None, y=None):
    """One mesh through the three entries against the yardstick; returns (got, yardstick, selection)."""
    g = np.random.default_rng(seed)
    verts = g.standard_normal((V, 3)).astype(np.float32)
    cols = g.random((V, 3)).astype(np.float32) if colors else None
    got = _raw(lib, dev, tris, V, verts, cols, mode, min_faces, min_ratio, guard)
    y = y if y is not None else _yardstick(tris, V)
    sel = _yard_select(tris, V, y, mode, min_faces, min_ratio)
    _check_components(got, y)
    _check_select(got, sel)
    _check_compact(got, tris, verts, cols, sel)
    return got, y, sel


# ---- the meshes ---------------------------------------------------------------------------------------------------------------------------------
def _strip(n):
    """n triangles (i, i+1, i+2) over n + 2 vertices: one component, a chain"""
    i = np.arange(n, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], axis=1)


def _sheet(nx, ny):
    """2 nx ny triangles over a grid of (nx + 1)(ny + 1) vertices"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    a = (i * (ny + 1) + j).reshape(-1)
    b, c, d = a + 1, a + ny + 1, a + ny + 2
    return np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int32)


_MANY = {}


def _many():
    """3000 disjoint triangles and one sheet of 4000 triangles, vertex ids and face order shuffled (seeded): (tris, V, yardstick, sheet ids)"""
    if not _MANY:
        g = np.random.default_rng(11)
        sheet = _sheet(40, 50)
        nsv = 41 * 51
        lone = (nsv + np.arange(9000, dtype=np.int32)).reshape(3000, 3)
        V = nsv + 9000
        ids = g.permutation(V).astype(np.int32)
        tris = ids[np.concatenate([sheet, lone])]
        tris = tris[g.permutation(len(tris))]
        _MANY.update(tris=tris, V=V, y=_yardstick(tris, V), sheet_ids=np.sort(ids[:nsv]))
    return _MANY["tris"], _MANY["V"], _MANY["y"], _MANY["sheet_ids"]


def _sparse(V, F, seed):
    """a random mesh of about V / 10 groups of vertices, every triangle inside one group (repeated corners and duplicates happen)"""
    g = np.random.default_rng(seed)
    ngroups = max(1, V // 10)
    group_of = g.integers(0, ngroups, V)
    group_of[:ngroups] = np.arange(ngroups)[:V]
    order = np.argsort(group_of, kind="stable")
    start = np.searchsorted(group_of[order], np.arange(ngroups))
    size = np.bincount(group_of, minlength=ngroups)
    fg = g.integers(0, ngroups, F)
    pick = (g.random((F, 3)) * size[fg][:, None]).astype(np.int64)
    return order[start[fg][:, None] + pick].astype(np.int32)


# ---- 1. edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_no_triangles_and_no_vertices(backend):
    lib, dev = _lib_and_dev(backend)
    none = np.zeros((0, 3), np.int32)
    got, y, _ = _full(lib, dev, none, 5)
    assert np.array_equal(got["labels"], np.arange(5)) and got["summary"].tolist() == [5, 0, -1, 0] and got["totals"].tolist() == [0, 0]
    assert np.array_equal(got["vertex_count"], np.ones(5)) and not got["face_count"].any()
    got, _, _ = _full(lib, dev, none, 5, mode=THRESHOLD)
    assert got["totals"].tolist() == [0, 0] and not got["keep_vertex"].any()
    got, _, _ = _full(lib, dev, none, 0)
    assert got["summary"].tolist() == [0, 0, -1, 0] and got["dropped"].tolist() == [0]
    got, _, _ = _full(lib, dev, [(0, 1, 2), (0, 0, 0)], 0)          # no vertex: every triangle is invalid
    assert got["summary"].tolist() == [0, 0, -1, 0] and got["dropped"].tolist() == [2] and got["totals"].tolist() == [0, 0]
    # the Python layer: empty arrays out
    v = torch.zeros(5, 3, device=dev)
    ov, ot, oc, info = meshops.clean_mesh(v, torch.zeros(0, 3, dtype=torch.int64, device=dev), colors=v, library=lib)
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and oc.shape == (0, 3) and ot.dtype == torch.int32 and ov.device.type == torch.device(dev).type
    assert info["n_components"] == 5 and info["largest_label"] == -1 and info["n_vertices"] == 0 and info["n_faces"] == 0
    cc = meshops.connected_components(torch.zeros(0, 3, dtype=torch.int32, device=dev), 0, library=lib)
    assert cc["n_components"] == 0 and cc["labels"].shape == (0,)


@pytest.mark.parametrize("backend", BACKENDS)
def test_small_meshes(backend):
    lib, dev = _lib_and_dev(backend)
    got, _, _ = _full(lib, dev, [(2, 4, 1)], 6)                                     # one triangle; vertices 0, 3, 5 unreferenced
    assert got["labels"].tolist() == [0, 1, 1, 3, 1, 5] and got["summary"].tolist() == [4, 1, 1, 1]
    assert got["out_triangles"].tolist() == [[1, 2, 0]] and got["totals"].tolist() == [3, 1]
    got, _, _ = _full(lib, dev, [(0, 1, 2), (2, 3, 4)], 5)                          # sharing exactly one vertex: one component
    assert got["summary"].tolist() == [1, 1, 0, 2] and got["totals"].tolist() == [5, 2]
    got, _, _ = _full(lib, dev, [(3, 4, 5), (0, 1, 2)], 6)                          # sharing none: a tie, the lower label wins
    assert got["summary"].tolist() == [2, 2, 0, 1] and got["keep_face"].tolist() == [0, 1] and got["out_triangles"].tolist() == [[0, 1, 2]]
    got, _, _ = _full(lib, dev, [(1, 1, 3), (4, 4, 4), (5, 3, 3)], 7)               # (a, a, b) triangles are valid and connect a and b
    assert got["labels"].tolist() == [0, 1, 2, 1, 4, 1, 6] and got["summary"].tolist() == [5, 2, 1, 2] and got["dropped"].tolist() == [0]
    got, _, _ = _full(lib, dev, [(0, 1, 2), (3, 4, 5), (3, 4, 5)], 6)               # a duplicate counts twice
    assert got["summary"].tolist() == [2, 2, 3, 2] and got["face_count"].tolist() == [1, 0, 0, 2, 0, 0]
    got, _, _ = _full(lib, dev, [(0, 1, 2), (3, 4, 5)], 6, mode=THRESHOLD)          # threshold 0: every component with a face
    assert got["totals"].tolist() == [6, 2]


@pytest.mark.parametrize("backend", BACKENDS)
def test_invalid_triangles_connect_nothing(backend):
    lib, dev = _lib_and_dev(backend)
    V = 8
    tris = [(0, 1, 2), (2, 3, V), (4, -1, 5), (5, 6, 7)]           # index V and index -1: (2, 3) and (4, 5) stay unconnected
    for mode in (LARGEST, THRESHOLD):
        got, y, _ = _full(lib, dev, tris, V, mode=mode)
        assert got["dropped"].tolist() == [2] and got["labels"].tolist() == [0, 0, 0, 3, 4, 5, 5, 5]
        assert got["keep_face"][1] == 0 and got["keep_face"][2] == 0 and got["face_map"][1] == -1 and got["face_map"][2] == -1
    assert got["totals"].tolist() == [6, 2] and got["out_triangles"].tolist() == [[0, 1, 2], [3, 4, 5]]
    tris64 = torch.tensor(tris, dtype=torch.int64, device=dev)
    tris64[1, 2] = 2 ** 32 + 1                                     # would wrap to the valid index 1 in int32: stays invalid
    cc = meshops.connected_components(tris64, V, library=lib)
    assert cc["dropped"] == 2 and cc["labels"].tolist() == [0, 0, 0, 3, 4, 5, 5, 5]


# ---- 2. long chains ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_long_chains(backend):
    """parent chains thousands long and compare-and-swap retries across many workgroups: a strip of 5000 triangles with descending vertex
    ids, with permuted ids, and with shuffled faces"""
    lib, dev = _lib_and_dev(backend)
    n, V = 5000, 5002
    g = np.random.default_rng(5)
    strip = _strip(n)
    perm = g.permutation(V).astype(np.int32)
    variants = {"descending": (V - 1 - strip).astype(np.int32), "permuted": perm[strip], "faces shuffled": strip[g.permutation(n)],
                "permuted, faces shuffled": perm[strip][g.permutation(n)]}
    labels = []
    for name, tris in variants.items():
        got, _, _ = _full(lib, dev, tris, V, colors=False)
        assert got["summary"].tolist() == [1, 1, 0, n] and not got["labels"].any(), name
        assert got["vertex_count"][0] == V and got["totals"].tolist() == [V, n], name
        labels.append(got["labels"])
    assert all(a.tobytes() == labels[0].tobytes() for a in labels)


# ---- 3. many components, the selection rules --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_many_components(backend):
    lib, dev = _lib_and_dev(backend)
    tris, V, y, sheet_ids = _many()
    got, _, sel = _full(lib, dev, tris, V, y=y)
    assert got["summary"].tolist() == [3001, 3001, int(sheet_ids[0]), 4000]
    assert np.array_equal(np.nonzero(got["keep_vertex"])[0], sheet_ids) and got["totals"].tolist() == [len(sheet_ids), 4000]
    for kw in (dict(min_faces=2), dict(min_ratio=1.0), dict(min_faces=4000), dict(min_faces=2, min_ratio=0.5)):      # 1.0f * 4000.0f = 4000: >= keeps it
        again, _, _ = _full(lib, dev, tris, V, mode=THRESHOLD, y=y, **kw)
        for k in OUT_KEYS:
            assert np.array_equal(again[k], got[k]), (kw, k)
    none, _, _ = _full(lib, dev, tris, V, mode=THRESHOLD, min_faces=4001, y=y)
    assert none["totals"].tolist() == [0, 0]
    every, _, _ = _full(lib, dev, tris, V, mode=THRESHOLD, min_faces=1, y=y)
    assert every["totals"].tolist() == [V, 7000]


@pytest.mark.parametrize("backend", BACKENDS)
def test_min_ratio_on_a_component_size(backend):
    """components of 8, 4, 2 and 1 faces: 0.5f * 8.0f = 4 and 0.25f * 8.0f = 2 are exact in fp32 and land on a size, which >= keeps; the
    next float above 0.5 gives ceil(4.0000005) = 5"""
    lib, dev = _lib_and_dev(backend)
    parts, base = [], 0
    for n in (1, 4, 8, 2):
        parts.append(_strip(n) + base)
        base += n + 2
    tris = np.concatenate(parts).astype(np.int32)
    above_half = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    for ratio, faces in ((0.5, 12), (0.25, 14), (above_half, 8), (0.125, 15), (1.0, 8), (0.0, 15)):
        got, _, _ = _full(lib, dev, tris, base, mode=THRESHOLD, min_ratio=ratio)
        assert got["totals"].tolist()[1] == faces, ratio
    got, _, _ = _full(lib, dev, tris, base, mode=THRESHOLD, min_ratio=0.25, min_faces=3)       # the larger of the two bounds
    assert got["totals"].tolist()[1] == 12


# ---- 4. block edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", EDGE_SIZES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_block_edges(backend, V):
    lib, dev = _lib_and_dev(backend)
    for F in EDGE_SIZES:
        tris = _sparse(V, F, seed=V * 10007 + F)
        _full(lib, dev, tris, V, mode=THRESHOLD, min_faces=2, seed=F)
    _full(lib, dev, _sparse(V, 300, seed=V), V, mode=LARGEST)


# ---- 5. compaction through the Python layer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_clean_mesh(backend):
    lib, dev = _lib_and_dev(backend)
    tris, V, y, sheet_ids = _many()
    g = np.random.default_rng(3)
    verts, cols = g.standard_normal((V, 3)), g.random((V, 3)).astype(np.float32)
    sel = _yard_select(tris, V, y, LARGEST)
    # float64 vertices, int64 triangles with strides (a transposed view), numpy colours
    t64 = torch.as_tensor(np.ascontiguousarray(tris.T).astype(np.int64)).to(dev).T
    assert not t64.is_contiguous()
    ov, ot, oc, info = meshops.clean_mesh(torch.as_tensor(verts).to(dev), t64, colors=cols, library=lib)
    assert ov.dtype == torch.float32 and ot.dtype == torch.int32 and oc.dtype == torch.float32 and not ov.requires_grad
    got = {"out_vertices": ov.cpu().numpy(), "out_colors": oc.cpu().numpy(), "out_triangles": ot.cpu().numpy()}
    _check_compact(got, tris, verts.astype(np.float32), cols, sel)
    assert (info["n_components"], info["n_components_with_faces"], info["largest_label"], info["largest_face_count"], info["dropped"]) == \
        (3001, 3001, int(sheet_ids[0]), 4000, 0)
    assert info["n_vertices"] == len(sheet_ids) and info["n_faces"] == 4000
    assert np.array_equal(info["vertex_map"].cpu().numpy(), sel["vertex_map"]) and np.array_equal(info["face_map"].cpu().numpy(), sel["face_map"])
    assert info["keep_vertex"].dtype == torch.bool and np.array_equal(info["keep_face"].cpu().numpy(), sel["keep_face"].astype(bool))
    for k in ("labels", "face_count", "vertex_count"):
        assert np.array_equal(info[k].cpu().numpy(), y[k]), k
    # no colours; cleaning a clean mesh is the identity
    pv, pt, pc, pinfo = meshops.clean_mesh(ov, ot, library=lib)
    assert pc is None and torch.equal(pv.view(torch.int32), ov.view(torch.int32)) and torch.equal(pt, ot)
    assert np.array_equal(pinfo["vertex_map"].cpu().numpy(), np.arange(len(sheet_ids))) and pinfo["n_components"] == 1
    # threshold mode through the same door; connected_components on its own
    tv, tt, _, tinfo = meshops.clean_mesh(torch.as_tensor(verts).to(dev), t64, keep="threshold", min_faces=2, library=lib)
    assert torch.equal(tv, ov) and torch.equal(tt, ot)
    cc = meshops.connected_components(t64, V, library=lib)
    assert cc["n_components_with_faces"] == 3001 and np.array_equal(cc["labels"].cpu().numpy(), y["labels"]) and cc["labels"].dtype == torch.int32
    assert cn.clean_mesh is meshops.clean_mesh and cn.connected_components is meshops.connected_components


def test_python_layer_refusals():
    lib = cn.load_library(N.EMU_LIB)
    v, t = torch.zeros(4, 3), torch.tensor([[0, 1, 2]])
    if os.path.isfile(cn.library_path()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            meshops.clean_mesh(v, t)                   # CPU tensors and the HIP library
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            meshops.connected_components(t, 4)
    with pytest.raises(ValueError, match="integer dtype"):
        meshops.clean_mesh(v, t.float(), library=lib)
    with pytest.raises(ValueError, match=r"\(F, 3\)"):
        meshops.connected_components(torch.zeros(3, 4, dtype=torch.int32), 4, library=lib)
    with pytest.raises(ValueError, match="floating-point"):
        meshops.clean_mesh(v.int(), t, library=lib)
    with pytest.raises(ValueError, match="expected 4 rows"):
        meshops.clean_mesh(v, t, colors=torch.zeros(3, 3), library=lib)
    with pytest.raises(ValueError, match="'largest' or 'threshold'"):
        meshops.clean_mesh(v, t, keep="biggest", library=lib)
    with pytest.raises(ValueError, match="takes no min_faces"):
        meshops.clean_mesh(v, t, min_faces=3, library=lib)
    with pytest.raises(ValueError, match="must not be negative"):
        meshops.clean_mesh(v, t, keep="threshold", min_ratio=float("nan"), library=lib)
    with pytest.raises(ValueError, match="must not be negative"):
        meshops.connected_components(t, -1, library=lib)


# ---- 6. through the product -------------------------------------------------------------------------------------------------------------------
RES = 32
CELL = 2.0 / (RES - 1)
SMALL_SPHERES = (((0.71, 0.66, 0.69), 0.13), ((-0.68, 0.07, -0.73), 0.1))


def _lattices():
    """u = -sdf on linspace(-1, 1, 32)^3: the sphere of radius 0.5 alone, and its union (max) with two small spheres far from it"""
    ax = np.linspace(-1.0, 1.0, RES, dtype=np.float32)
    x, yy, z = np.meshgrid(ax, ax, ax, indexing="ij")
    big = (np.float32(0.5) - np.sqrt(x * x + yy * yy + z * z)).astype(np.float32)
    union = big.copy()
    for (cx, cy, cz), r in SMALL_SPHERES:
        union = np.maximum(union, (np.float32(r) - np.sqrt((x - cx) ** 2 + (yy - cy) ** 2 + (z - cz) ** 2)).astype(np.float32))
    return torch.from_numpy(big), torch.from_numpy(union)


def _tiny_renderer(lib, dev):
    fx = G.load("tiny_sharp")
    ocfg, P = G.weights_of("tiny_sharp", fx)
    return N.make_renderer(ocfg, P, lib, dev)


def test_the_lattice_of_the_product_case_has_three_separate_shells():
    """the precondition of the next test, on the emulation: three components, the small ones at least two cells from everything else"""
    lib = cn.load_library(N.EMU_LIB)
    r = _tiny_renderer(lib, "cpu")
    _, union = _lattices()
    verts, tris = r.marching_cubes(union, [-1.0] * 3, [1.0] * 3)
    cc = meshops.connected_components(tris, verts.shape[0], library=lib)
    assert cc["n_components"] == 3 and cc["n_components_with_faces"] == 3 and cc["dropped"] == 0
    labels, v = cc["labels"].numpy(), verts.numpy().astype(np.float64)
    roots = np.unique(labels)
    sizes = sorted(int(cc["face_count"][int(x)]) for x in roots)
    assert sizes[0] >= 8 and sizes[2] == cc["largest_face_count"] and sizes[2] > 10 * sizes[1]
    for a in roots:
        for b in roots:
            if a < b:
                d = np.sqrt(((v[labels == a][:, None, :] - v[labels == b][None, :, :]) ** 2).sum(-1)).min()
                assert d >= 4 * CELL, (a, b, d / CELL)


@pytest.mark.parametrize("backend", BACKENDS)
def test_through_the_product(backend):
    """clean_mesh(marching_cubes(big sphere + two floaters)) IS marching_cubes(big sphere), bit for bit: the cells are independent and the
    compaction keeps the order.  render_mesh_view / extract_geometry with clean="largest" give the same mesh; clean=None is today's path."""
    lib, dev = _lib_and_dev(backend)
    r = _tiny_renderer(lib, dev)
    big, union = (u.to(dev) for u in _lattices())
    bmin, bmax = [-1.0] * 3, [1.0] * 3
    want_v, want_t = r.marching_cubes(big, bmin, bmax)
    raw_v, raw_t = r.marching_cubes(union, bmin, bmax)
    assert raw_t.shape[0] > want_t.shape[0] > 500
    ov, ot, _, info = meshops.clean_mesh(raw_v, raw_t, library=lib)
    assert info["n_components"] == 3 and torch.equal(ov.view(torch.int32), want_v.view(torch.int32)) and torch.equal(ot, want_t)
    tv, tt, _, _ = meshops.clean_mesh(raw_v, raw_t, keep="threshold", min_ratio=0.5, library=lib)
    assert torch.equal(tv.view(torch.int32), want_v.view(torch.int32)) and torch.equal(tt, want_t)

    r.extract_fields = lambda *a, **k: union              # the renderer's lattice for the calls below (its own network draws no floaters)
    cam = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -3.0], [0.0, 0.0, 0.0, 1.0]], device=dev)
    foc = torch.tensor([60.0, 60.0], device=dev)
    view = r.render_mesh_view(bmin, bmax, RES, cam, foc, 36, 48, clean="largest")
    assert torch.equal(view["triangles"], want_t) and torch.equal(view["vertices"].view(torch.int32), want_v.view(torch.int32))
    assert view["colors"].shape == want_v.shape and torch.equal(view["colors"].view(torch.int32), r.vertex_colors(want_v).view(torch.int32))
    assert view["dropped"] == {"behind_or_far": 0, "bad_index": 0} and bool(view["mask"].any())
    for clean in ("largest", dict(keep="threshold", min_ratio=0.5)):
        gv, gt = r.extract_geometry(bmin, bmax, dev, RES, clean=clean)
        assert gv.dtype == np.float64 and gt.dtype == np.int64
        assert np.array_equal(gv, want_v.cpu().numpy().astype(np.float64)) and np.array_equal(gt, want_t.cpu().numpy().astype(np.int64))

    # clean=None: the call without the argument, and the pieces put together by hand as before this feature
    plain, none = r.render_mesh_view(bmin, bmax, RES, cam, foc, 36, 48), r.render_mesh_view(bmin, bmax, RES, cam, foc, 36, 48, clean=None)
    colors = r.vertex_colors(raw_v)
    hand = cn.rasterize_mesh(raw_v, raw_t, cam, foc, 36, 48, colors=colors, library=lib)
    hand.update(vertices=raw_v, triangles=raw_t, colors=colors)
    assert list(plain) == list(none) == list(hand)
    for k in hand:
        for other in (plain, none):
            if torch.is_tensor(hand[k]):
                a, b = hand[k].cpu().contiguous().numpy(), other[k].cpu().contiguous().numpy()
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
            else:
                assert hand[k] == other[k], k
    assert bool((plain["tri_id"] != view["tri_id"]).any())       # the floaters are on screen without the clean-up
    pv, pt = r.extract_geometry(bmin, bmax, dev, RES)
    assert np.array_equal(pv, raw_v.cpu().numpy().astype(np.float64)) and np.array_equal(pt, raw_t.cpu().numpy().astype(np.int64))


# ---- 7. guarded buffers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("backend", BACKENDS)
def test_guarded_buffers(backend, fill):
    """every typed output an exact-size payload, poisoned, between guard bytes, the inputs between NaN guards: the same bits as the plain run,
    no guard byte touched (no entry reads an output before it wrote it, none reaches past V, F, V' or F')"""
    lib, dev = _lib_and_dev(backend)
    tris, V, y, _ = _many()
    for mode, kw in ((LARGEST, {}), (THRESHOLD, dict(min_faces=1))):
        plain, _, _ = _full(lib, dev, tris, V, mode=mode, y=y, **kw)
        guard = _guard.Guard(fill)
        got, _, _ = _full(lib, dev, tris, V, mode=mode, y=y, guard=guard, **kw)
        assert len(guard.regions) == 16
        for k in OUT_KEYS:
            assert got[k].tobytes() == plain[k].tobytes(), k
    guard = _guard.Guard(fill)                       # empty inputs and outputs still have a place between their guards
    _full(lib, dev, np.zeros((0, 3), np.int32), 3, guard=guard)
    _full(lib, dev, [(0, 1, 2)], 0, guard=guard)


# ---- 8. the entries' refusals; binding ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_refusals(backend):
    lib, dev = _lib_and_dev(backend)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    p, null, stream = _lib.ptr, C.c_void_p(0), _lib.stream_of(torch.device(dev))
    t, a, b, c, summary, dropped = i32(3).reshape(1, 3), i32(4), i32(4), i32(4), i32(6), i32(1)
    u8 = torch.zeros(4, dtype=torch.uint8, device=dev)
    big = 2 ** 31
    lib.timing_enable(True)
    try:
        lib.timing_collect()
        for args, msg in (((p(t), big, 4, p(a), p(b), p(c), p(summary), p(dropped), stream), "must not exceed"),
                          ((p(t), 1, big, p(a), p(b), p(c), p(summary), p(dropped), stream), "must not exceed"),
                          ((p(t), -1, 4, p(a), p(b), p(c), p(summary), p(dropped), stream), "negative"),
                          ((null, 1, 4, p(a), p(b), p(c), p(summary), p(dropped), stream), "null argument"),
                          ((p(t), 1, 4, p(a), null, p(c), p(summary), p(dropped), stream), "null argument"),
                          ((p(t), 1, 4, p(a), p(b), p(c), null, p(dropped), stream), "null argument"),
                          ((p(t), 1, 4, p(a), p(b), p(c), C.c_void_p(summary.data_ptr() + 4), p(dropped), stream), "8-byte aligned")):
            with pytest.raises(RuntimeError, match=msg):
                lib.call("cnr_mesh_components", *args)
        sel = lambda **kw: (p(t), kw.get("F", 1), kw.get("V", 4), p(a), p(b), p(summary), kw.get("mode", 0), kw.get("min_faces", 0),
                            kw.get("min_ratio", 0.0), kw.get("kv", p(u8)), p(u8), p(c), p(c), kw.get("totals", p(dropped)), stream)
        for kw, msg in ((dict(F=big), "must not exceed"), (dict(mode=2), "mode must be"), (dict(min_faces=-1), "must not be negative"),
                        (dict(min_ratio=-0.5), "must not be negative"), (dict(min_ratio=float("nan")), "must not be negative"),
                        (dict(kv=null), "null argument"), (dict(totals=null), "null argument")):
            with pytest.raises(RuntimeError, match=msg):
                lib.call("cnr_mesh_select", *sel(**kw))
        f = torch.zeros(4, 3, device=dev)
        for args, msg in (((p(f), null, p(t), 1, big, p(a), p(c), p(f), null, p(t), stream), "must not exceed"),
                          ((p(f), p(f), p(t), 1, 4, p(a), p(c), p(f), null, p(t), stream), "null together"),
                          ((null, null, p(t), 1, 4, p(a), p(c), p(f), null, p(t), stream), "null argument"),
                          ((p(f), null, p(t), 1, 4, p(a), null, p(f), null, p(t), stream), "null argument")):
            with pytest.raises(RuntimeError, match=msg):
                lib.call("cnr_mesh_compact", *args)
        assert lib.timing_collect() == []          # nothing was launched after a refusal
    finally:
        lib.timing_enable(False)
    assert lib.lib.cnr_abi_version() == _lib.ABI_VERSION


def test_header_binding_and_sources_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "colorneus_render.h")).read()
    ops = open(os.path.join(root, "color-neus_amd", "csrc", "cnr_ops.cpp")).read()
    for name, nargs in (("cnr_mesh_components", 9), ("cnr_mesh_select", 15), ("cnr_mesh_compact", 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is C.c_int
        assert header.count("int %s(" % name) == 1 and ops.count("\nint %s(" % name) == 1
    assert not [n for n in _lib.SIGNATURES if n.startswith("cnr_mesh_c") and n.endswith("_bytes")]      # no size query: typed buffers only
    src = open(os.path.join(root, "color-neus_amd", "csrc", "cnr_meshcc.h")).read()
    assert "constexpr int kMeshScanThreads = 1024, kMeshScanPer = 8;" in src and SCAN_CHUNK == 1024 * 8

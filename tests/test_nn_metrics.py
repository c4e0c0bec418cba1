"""Exact nearest-neighbour search (cnr_nn_search) and the mesh metrics on top of it (color_neus_amd.metrics, meshio.read_ply_vertices).

Every case runs on the CPU-emulation library (device cpu) and, marked gpu, on the HIP library (cuda:0).  The yardsticks are written here
and use nothing from the library:

  R32   the specified arithmetic restated in plain float32 torch on the CPU: dx = a[..., 0] - b[..., 0] etc., then (dx*dx + dy*dy) + dz*dz as
        separate element-wise operations (each is one IEEE rounding, so this is the specification bit for bit), then d.min(dim=1), which
        torch documents as returning the first minimal index.  The library must match it BITWISE in dist2 and exactly in idx.
  R64   the same in float64 on the float32 inputs.  Bound 1e-6 relative: the formula has five roundings on non-negative terms plus the
        rounded differences, a relative error below 6 * 2^-24 = 3.6e-7.
"""
import os

import numpy as np
import pytest
import torch

import color_neus_amd as cn
import _native as N

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return N.EMU_LIB, "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return None, "cuda:0"


def _d2(a, b):
    """All-pairs (dx*dx + dy*dy) + dz*dz in the dtype of a / b, one rounding per operation."""
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def _ref(q, t, dtype, chunk=512):
    """(min_j d2, first argmin) per query, by chunks of queries (bounded memory)."""
    q, t = q.detach().cpu().to(dtype), t.detach().cpu().to(dtype)
    ds, js = [], []
    for s in range(0, q.shape[0], chunk):
        d, j = _d2(q[s:s + chunk], t).min(dim=1)
        ds.append(d)
        js.append(j)
    return torch.cat(ds), torch.cat(js)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _assert_bitwise_r32(q, t, dist2, idx):
    d32, j32 = _ref(q.float(), t.float(), torch.float32)
    assert dist2.dtype == torch.float32 and idx.dtype == torch.int64
    assert torch.equal(_bits(dist2), _bits(d32)), int((_bits(dist2) != _bits(d32)).sum())
    assert torch.equal(idx.cpu(), j32), int((idx.cpu() != j32).sum())


def _assert_r64_bounds(q, t, dist2, idx):
    q64, t64 = q.detach().cpu().float().double(), t.detach().cpu().float().double()
    d64, _ = _ref(q64, t64, torch.float64)
    err = ((dist2.cpu().double() - d64).abs() / d64).max().item()
    diff = q64 - t64[idx.cpu()]
    chosen = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
    excess = (chosen / d64).max().item() - 1.0
    print(f"R64: max relative dist2 error {err:.3e}, chosen-index excess {excess:.3e}")
    assert ((dist2.cpu().double() - d64).abs() <= 1e-6 * d64).all(), err
    assert (chosen <= (1.0 + 1e-6) * d64).all(), excess


def _case1():
    g = torch.Generator().manual_seed(0)
    q = torch.rand(5000, 3, generator=g) * 2 - 1
    t = torch.rand(7001, 3, generator=g) * 2 - 1
    return q, t


@pytest.mark.parametrize("backend", BACKENDS)
def test_random_clouds_bitwise_r32_and_within_r64_bounds(backend):
    lib, dev = _lib_and_dev(backend)
    q, t = _case1()
    dist2, idx = cn.metrics.nearest_neighbors(q.to(dev), t.to(dev), library=lib)
    assert dist2.shape == (5000,) and idx.shape == (5000,) and dist2.device.type == torch.device(dev).type
    _assert_bitwise_r32(q, t, dist2, idx)
    _assert_r64_bounds(q, t, dist2, idx)


def _tie_case():
    ax = torch.linspace(-1, 1, 9)
    lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    g = torch.Generator().manual_seed(1)
    t = torch.cat([lat, lat[torch.randperm(lat.shape[0], generator=g)[:200]]])      # exact duplicates at higher indices
    mid = (lat[:-1] + lat[1:]) * 0.5                                                # midpoints of consecutive lattice points
    q = torch.cat([lat[torch.randperm(lat.shape[0], generator=g)[:100]], mid[torch.randperm(mid.shape[0], generator=g)[:300]], torch.zeros(1, 3)])
    return q, t


@pytest.mark.parametrize("backend", BACKENDS)
def test_exact_ties_go_to_the_lowest_index(backend):
    lib, dev = _lib_and_dev(backend)
    q, t = _tie_case()
    assert q.shape[0] == 401 and t.shape[0] == 929
    d = _d2(q, t)
    tied = int(((d == d.min(dim=1, keepdim=True).values).sum(dim=1) > 1).sum())
    assert tied >= 250, tied          # the lowest-index rule decides most of the queries
    dist2, idx = cn.metrics.nearest_neighbors(q.to(dev), t.to(dev), library=lib)
    _assert_bitwise_r32(q, t, dist2, idx)


@pytest.mark.parametrize("backend", BACKENDS)
def test_few_queries_many_targets(backend):
    """37 x 500 003: the target range is split over many workgroups."""
    lib, dev = _lib_and_dev(backend)
    g = torch.Generator().manual_seed(2)
    q = torch.rand(37, 3, generator=g) * 2 - 1
    t = torch.rand(500003, 3, generator=g) * 2 - 1
    dist2, idx = cn.metrics.nearest_neighbors(q.to(dev), t.to(dev), library=lib)
    _assert_bitwise_r32(q, t, dist2, idx)


# query counts at one workgroup's load (256 threads x 4 queries) and that +- 1; target counts at one LDS tile (1024) and that +- 1
# (test_edges runs 1 x 1 and 300 x 400: no pair of these)
QUERIES_PER_WORKGROUP = TARGETS_PER_TILE = 1024
SHAPES = [(QUERIES_PER_WORKGROUP - 1, 1500), (QUERIES_PER_WORKGROUP, 1500), (QUERIES_PER_WORKGROUP + 1, 1500),
          (100, TARGETS_PER_TILE - 1), (100, TARGETS_PER_TILE), (100, TARGETS_PER_TILE + 1)]


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_launch_shapes(backend, n, m):
    """R32, bitwise."""
    lib, dev = _lib_and_dev(backend)
    g = torch.Generator().manual_seed(1000 * n + m)
    q = torch.rand(n, 3, generator=g) * 2 - 1
    t = torch.rand(m, 3, generator=g) * 2 - 1
    dist2, idx = cn.metrics.nearest_neighbors(q.to(dev), t.to(dev), library=lib)
    _assert_bitwise_r32(q, t, dist2, idx)


@pytest.mark.parametrize("backend", BACKENDS)
def test_edges(backend):
    lib, dev = _lib_and_dev(backend)
    nn = cn.metrics.nearest_neighbors
    # n = m = 1
    dist2, idx = nn(torch.tensor([[0.5, -1.0, 2.0]], device=dev), torch.tensor([[0.0, 1.0, 2.0]], device=dev), library=lib)
    assert dist2.tolist() == [4.25] and idx.tolist() == [0]
    # n = 0 / m = 0
    q, t = _case1()
    q, t = q[:300].to(dev), t[:400].to(dev)
    dist2, idx = nn(q[:0], t, library=lib)
    assert dist2.shape == (0,) and idx.shape == (0,) and dist2.dtype == torch.float32 and idx.dtype == torch.int64
    with pytest.raises(ValueError):
        nn(q, t[:0], library=lib)
    base_d, base_i = nn(q, t, library=lib)
    _assert_bitwise_r32(q, t, base_d, base_i)
    # float64, non-contiguous and requires_grad inputs: the result of their contiguous float32 copies, no graph
    q_nc = torch.zeros(300, 6, device=dev)[:, ::2]
    q_nc.copy_(q)
    t_t = t.t().contiguous().t()
    assert not q_nc.is_contiguous() and not t_t.is_contiguous()
    for qq, tt in ((q.double(), t.double()), (q_nc, t_t), (q.clone().requires_grad_(True), t.clone().requires_grad_(True))):
        d, i = nn(qq, tt, library=lib)
        assert torch.equal(_bits(d), _bits(base_d)) and torch.equal(i, base_i)
        assert d.grad_fn is None and not d.requires_grad and i.grad_fn is None
    # a NaN target appended as the LAST target changes nothing
    t_nan = torch.cat([t, torch.tensor([[0.0, float("nan"), 0.0]], device=dev)])
    d, i = nn(q, t_nan, library=lib)
    assert torch.equal(_bits(d), _bits(base_d)) and torch.equal(i, base_i)
    # a NaN query: idx -1 and a NaN distance; the other queries are untouched
    q_nan = q.clone()
    q_nan[7, 2] = float("nan")
    d, i = nn(q_nan, t, library=lib)
    assert i[7].item() == -1 and torch.isnan(d[7]).item()
    keep = torch.arange(300, device=dev) != 7
    assert torch.equal(_bits(d[keep]), _bits(base_d[keep])) and torch.equal(i[keep], base_i[keep])


@pytest.mark.parametrize("backend", BACKENDS)
def test_overflowing_distances(backend):
    """d2 == +inf is an ordinary candidate (above every finite value, below NaN): the search takes it through its own branch, so it gets its
    own input.  Query 0 overflows against every target (first +inf wins: R32's first minimal index); query 1 overflows against all but one;
    query 2 sees NaN (inf - inf) against target 0, +inf against the others; the first +inf sits behind 1500 NaN targets for query 3."""
    lib, dev = _lib_and_dev(backend)
    big = 3.0e38
    t = torch.zeros(3000, 3)
    t[:, 0] = torch.linspace(-1, 1, 3000)
    t[0] = torch.tensor([float("inf"), 0.0, 0.0])
    t[2500] = torch.tensor([big, big, 0.0])
    q = torch.tensor([[-big, 0.0, 0.0], [big, big, 1.0], [float("inf"), 0.0, 0.0]])
    dist2, idx = cn.metrics.nearest_neighbors(q.to(dev), t.to(dev), library=lib)
    d = _d2(q, t)
    assert torch.isinf(d[0]).all() and torch.isnan(d[2, 0]) and torch.isinf(d[2, 1:]).all()
    assert idx.tolist() == [0, 2500, 1] and dist2.tolist() == [float("inf"), 1.0, float("inf")]
    t2 = torch.cat([torch.full((1500, 3), float("nan")), t[1:]])
    dist2, idx = cn.metrics.nearest_neighbors(q[:1].to(dev), t2.to(dev), library=lib)
    assert idx.tolist() == [1500] and dist2.tolist() == [float("inf")]


def _normalize64(pc):
    pc = pc.double()
    pc = pc - pc.mean(dim=0)
    return pc / pc.pow(2).sum(dim=1).sqrt().max()


def _chamfer64(x, y):
    dxy, _ = _ref(x, y, torch.float64)
    dyx, _ = _ref(y, x, torch.float64)
    return dxy, dyx


@pytest.mark.parametrize("backend", BACKENDS)
def test_chamfer_distance(backend):
    lib, dev = _lib_and_dev(backend)
    x, y = _case1()
    dxy, dyx = _chamfer64(x, y)
    ref = (dxy.mean() + dyx.mean()).item()
    cd = cn.metrics.chamfer_distance(x.to(dev), y.to(dev), library=lib)
    assert cd.dtype == torch.float64 and cd.dim() == 0 and cd.grad_fn is None
    print(f"chamfer: {cd.item():.12e} vs R64 {ref:.12e}, relative {abs(cd.item() - ref) / ref:.2e}")
    assert abs(cd.item() - ref) <= 1e-6 * ref
    # norm=True: R64 on clouds normalised in float64 from the float32 inputs.  rtol 1e-5: the library normalises in float32 (two more roundings
    # per coordinate of a unit-size cloud whose nearest-neighbour distances are about 0.05: up to ~1e-5 on a single pair, far less on the mean)
    dxy, dyx = _chamfer64(_normalize64(x), _normalize64(y))
    ref = (dxy.mean() + dyx.mean()).item()
    cdn = cn.metrics.chamfer_distance(x.to(dev), y.to(dev), norm=True, library=lib)
    print(f"chamfer norm=True: {cdn.item():.12e} vs R64 {ref:.12e}, relative {abs(cdn.item() - ref) / ref:.2e}")
    assert abs(cdn.item() - ref) <= 1e-5 * ref
    assert cn.chamfer_distance is cn.metrics.chamfer_distance


@pytest.mark.parametrize("backend", BACKENDS)
def test_mesh_metrics(backend):
    lib, dev = _lib_and_dev(backend)
    pred, gt = _case1()
    taus = (0.02, 0.05, 0.1)
    d_pg, d_gp = (d.sqrt() for d in _chamfer64(pred, gt))
    for tau in taus:      # precondition: no distance so close to a threshold that a float32 rounding (<= 2e-7 relative on d) could flip a count
        gap = min(((d_pg - tau).abs() / tau).min().item(), ((d_gp - tau).abs() / tau).min().item())
        assert gap > 1e-5, (tau, gap)
    m = cn.metrics.mesh_metrics(pred.to(dev), gt.to(dev), thresholds=taus, library=lib)
    assert all(type(v) is float for v in m.values())
    for k, ref in (("accuracy", d_pg.mean().item()), ("completeness", d_gp.mean().item()),
                   ("chamfer_l1", 0.5 * (d_pg.mean().item() + d_gp.mean().item()))):
        assert abs(m[k] - ref) <= 1e-6 * ref, (k, m[k], ref)
    assert m["chamfer_l2"] == cn.metrics.chamfer_distance(pred.to(dev), gt.to(dev), library=lib).item()
    for tau in taus:
        p, r = int((d_pg < tau).sum()) / 5000, int((d_gp < tau).sum()) / 7001
        assert 0.01 < p < 0.99 and 0.01 < r < 0.99          # no threshold is trivial
        assert m[f"precision@{tau:g}"] == p and m[f"recall@{tau:g}"] == r, (tau, m, p, r)
        assert m[f"fscore@{tau:g}"] == 2.0 * p * r / (p + r)
    far = cn.metrics.mesh_metrics(pred.to(dev), gt.to(dev) + 10.0, thresholds=(0.1,), library=lib)
    assert far["precision@0.1"] == 0.0 and far["recall@0.1"] == 0.0 and far["fscore@0.1"] == 0.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_cloud_against_itself(backend):
    lib, dev = _lib_and_dev(backend)
    x = _case1()[0].to(dev)
    assert cn.metrics.chamfer_distance(x, x, library=lib).item() == 0.0
    dist2, idx = cn.metrics.nearest_neighbors(x, x, library=lib)
    assert torch.equal(idx.cpu(), torch.arange(5000)) and not dist2.any()


@pytest.mark.parametrize("backend", BACKENDS)
def test_ply_files(backend, tmp_path):
    lib, dev = _lib_and_dev(backend)
    rng = np.random.default_rng(0)
    va, vb, vc, vd = (rng.uniform(-1, 1, (n, 3)).astype(np.float32) for n in (500, 700, 60, 333))
    tri = rng.integers(0, 500, (40, 3))
    pa, pb, pc, pd = (str(tmp_path / f"{n}.ply") for n in "abcd")
    cn.write_ply(pa, va, tri)
    cn.write_ply(pb, vb, tri, colors=rng.uniform(0, 1, (700, 3)))
    with open(pc, "w") as fh:       # ASCII, normals behind the positions, a comment, no face element
        fh.write("ply\nformat ascii 1.0\ncomment hand written\nelement vertex 60\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nend_header\n")
        for v in vc:
            fh.write(" ".join(repr(float(c)) for c in v) + " 0 0 1\n")
    rec = np.zeros(333, dtype=[("nx", "<f4"), ("x", "<f8"), ("red", "u1"), ("y", "<f8"), ("z", "<f8"), ("ny", "<f4"), ("nz", "<i2")])
    rec["x"], rec["y"], rec["z"], rec["nx"], rec["red"] = vd[:, 0], vd[:, 1], vd[:, 2], 1.0, 7
    with open(pd, "wb") as fh:      # binary, double positions interleaved with other scalar properties, no face element
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 333\nproperty float nx\nproperty double x\nproperty uchar red\n"
                 b"property double y\nproperty double z\nproperty float ny\nproperty short nz\nend_header\n")
        fh.write(rec.tobytes())
    for path, v in ((pa, va), (pb, vb), (pc, vc), (pd, vd)):
        got = cn.meshio.read_ply_vertices(path)
        assert got.dtype == np.float32 and got.shape == v.shape and np.array_equal(got, v), path
    for src, tgt, a, b in ((pa, pb, va, vb), (pc, pd, vc, vd)):
        for norm in (False, True):
            on_files = cn.metrics.compute_chamfer_distance(src, tgt, device=dev, norm=norm, library=lib)
            on_arrays = cn.metrics.chamfer_distance(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), norm=norm, library=lib)
            assert on_files.item() == on_arrays.item() and on_files.item() > 0


def test_cpu_points_need_an_emulation_library():
    """No CPU fallback: CPU tensors with the HIP library (the default) are an error, not a torch computation."""
    if not os.path.isfile(cn.library_path()):
        pytest.skip("HIP library not built")
    q, t = _case1()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.metrics.nearest_neighbors(q, t)


def test_abi_argument_checks():
    import ctypes as C
    lib = cn.load_library(N.EMU_LIB)
    L = lib.lib
    assert L.cnr_abi_version() == 9
    q = torch.zeros(4, 3)
    d, i = torch.empty(4), torch.empty(4, dtype=torch.int32)
    nb = L.cnr_nn_scratch_bytes(4, 4)
    assert nb >= 32 and L.cnr_nn_scratch_bytes(0, 4) == 0
    s = torch.empty(nb, dtype=torch.uint8)
    p = lambda x: C.c_void_p(x.data_ptr())
    assert L.cnr_nn_search(p(q), 4, p(q), 4, p(d), p(i), p(s), nb, None) == 0
    assert L.cnr_nn_search(None, 0, None, 0, None, None, None, 0, None) == 0          # n_query == 0: a no-op
    for args, msg in (((p(q), 4, p(q), 0, p(d), p(i), p(s), nb, None), "target"), ((p(q), 4, p(q), 1 << 31, p(d), p(i), p(s), nb, None), "2^31"),
                      ((p(q), 4, None, 4, p(d), p(i), p(s), nb, None), "null"), ((p(q), 4, p(q), 4, p(d), p(i), p(s), nb - 1, None), "scratch")):
        assert L.cnr_nn_search(*args) < 0
        assert msg in L.cnr_last_error().decode(), L.cnr_last_error().decode()


@pytest.mark.gpu
def test_hip_matches_the_emulation_bitwise_at_2_17():
    """2^17 x (2^17 + 3) seeded normal clouds: HIP against the emulation library on the CPU, bitwise; the R64 bounds on a fixed subset of 2048
    queries; one call on a non-default stream gives the same bits."""
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator().manual_seed(17)
    q = torch.randn(1 << 17, 3, generator=g)
    t = torch.randn((1 << 17) + 3, 3, generator=g)
    d_emu, i_emu = cn.metrics.nearest_neighbors(q, t, library=N.EMU_LIB)
    qd, td = q.cuda(), t.cuda()
    d_hip, i_hip = cn.metrics.nearest_neighbors(qd, td)
    assert torch.equal(_bits(d_hip), _bits(d_emu)), int((_bits(d_hip) != _bits(d_emu)).sum())
    assert torch.equal(i_hip.cpu(), i_emu), int((i_hip.cpu() != i_emu).sum())
    sub = torch.arange(2048) * 64
    _assert_r64_bounds(q[sub], t, d_hip.cpu()[sub], i_hip.cpu()[sub])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d_s, i_s = cn.metrics.nearest_neighbors(qd, td)
    side.synchronize()
    assert torch.equal(_bits(d_s), _bits(d_emu)) and torch.equal(i_s.cpu(), i_emu)

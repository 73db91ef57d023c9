"""sugar_dynamic (include/gsr.h gsr_sugar_skin_*, gsr_sugar_timed_*) without a GPU: the properties that pin the fp64
restatement of tests/sugar_dynamic_reference.py (the checker of the GPU tests), the skin binding's incidence and its
Euclidean constructor, and the argument checks of the Python wrappers and of the C entries (which precede any device
work).  The kernels' numerics are checked on the GPU in tests/test_gpu_sugar_dynamic.py."""
import ctypes
import math

import pytest

from diff_gaussian_rasterization import _C

torch = pytest.importorskip("torch")

import gsr_synthetic as gs  # noqa: E402
import sugar_dynamic  # noqa: E402
import sugar_dynamic_reference as ref  # noqa: E402
from sugar_dynamic import SkinBinding, skin_vertices, timed_gaussians  # noqa: E402
from sugar_cases import random_quats  # noqa: E402
from sugar_mesh import MeshBinding  # noqa: E402

NAMES = ("gsr_sugar_skin_workspace_bytes", "gsr_sugar_skin_forward", "gsr_sugar_skin_backward",
         "gsr_sugar_timed_workspace_bytes", "gsr_sugar_timed_forward", "gsr_sugar_timed_backward")
D = torch.float64


def test_library_has_the_entry_points_at_abi_9():
    lib = _C.load_library()
    assert _C.ABI_VERSION == 9 and lib.gsr_abi_version() == 9
    for name in NAMES:
        assert hasattr(lib, name) and name in _C.SIGNATURES


# ---- the restatement ----------------------------------------------------------------------------------------------
def test_exp_of_log_is_the_unit_quaternion_up_to_sign():
    gen = torch.Generator().manual_seed(0)
    q = random_quats(gen, (500,), D, max_angle=3.1)
    back = ref.qexp(ref.qlog(q))
    unit = q / q.norm(dim=-1, keepdim=True)
    sign = torch.where(unit[:, 3:] < 0, -1.0, 1.0).to(D)  # Exp yields w >= 0
    assert float((back - sign * unit).abs().max()) < 1e-14
    assert (back[:, 3] >= 0).all()
    # scale invariance, Log(q) = Log(-q), |theta| <= pi, theta = pi at w = 0
    assert float((ref.qlog(3.7 * q) - ref.qlog(q)).abs().max()) < 1e-14
    assert float((ref.qlog(-q) - ref.qlog(q)).abs().max()) < 1e-14
    assert float(ref.qlog(q).norm(dim=-1).max()) <= math.pi + 1e-14
    half = ref.qlog(torch.tensor([[0.0, 2.0, 0.0, 0.0]], dtype=D))
    assert torch.allclose(half, torch.tensor([[0.0, math.pi, 0.0]], dtype=D), atol=1e-15)
    # the series joins the closed form
    for dtype, r in ((D, 0.9e-4), (D, 1.1e-4), (torch.float32, 0.9e-2), (torch.float32, 1.1e-2)):
        v = torch.tensor([[r * 0.6, 0.0, r * 0.8, 1.0]], dtype=dtype) * 1.3
        want = 2 * math.atan(r) / r * torch.tensor([[r * 0.6, 0.0, r * 0.8]], dtype=D)
        assert float((ref.qlog(v).double() - want).abs().max()) <= 8 * torch.finfo(dtype).eps * r
        phi = torch.tensor([[r * 0.6, 0.0, r * 0.8]], dtype=dtype)
        want = torch.tensor([[math.sin(r / 2) * 0.6, 0.0, math.sin(r / 2) * 0.8, math.cos(r / 2)]], dtype=D)
        assert float((ref.qexp(phi).double() - want).abs().max()) <= 2 * torch.finfo(dtype).eps


def test_log_at_the_identity_and_its_gradient():
    for w in (1.0, 0.5, -2.0):
        q = torch.tensor([[0.0, 0.0, 0.0, w]], dtype=D, requires_grad=True)
        phi = ref.qlog(q)
        assert torch.equal(phi, torch.zeros(1, 3, dtype=D))
        jac = torch.autograd.functional.jacobian(lambda x: ref.qlog(x)[0], q)[:, 0]  # (3, 4)
        want = torch.cat([2 / w * torch.eye(3, dtype=D), torch.zeros(3, 1, dtype=D)], 1)
        assert torch.equal(jac, want)
    one = ref.qexp(torch.zeros(1, 3, dtype=D))
    assert torch.equal(one, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=D))


def _graph(gen, V=30, P=6, K=4, T=2, dtype=D):
    verts = torch.randn(V, 3, generator=gen, dtype=D).to(dtype)
    node_xyz = torch.randn(P, 3, generator=gen, dtype=D).to(dtype)
    b = SkinBinding.from_euclidean(verts, node_xyz, K)
    return verts, node_xyz, b


@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_equal_nodes_give_a_rigid_motion(method):
    gen = torch.Generator().manual_seed(1)
    verts, node_xyz, b = _graph(gen)
    T, P = 2, b.n_nodes
    q = random_quats(gen, (T, 1), D, identity_every=0).expand(T, P, 4).contiguous()
    trans = torch.randn(T, 1, 3, generator=gen, dtype=D).expand(T, P, 3).contiguous()
    w = b.w.double() / b.w.double().sum(-1, keepdim=True)
    xyz, rot, scale = ref.skin_vertices_reference(verts, node_xyz, trans, q, b.nbr.long(), w, method)
    qh = q[:, :1] / q[:, :1].norm(dim=-1, keepdim=True)
    R = ref.qmatrix(qh)  # (T, 1, 3, 3)
    if method == "dqs":
        want = (R @ verts[None, :, :, None])[..., 0] + trans[:, :1]
    else:  # each node turns the vertex about itself: the weighted node centre stays out of the rotation
        xbar = (w[..., None] * node_xyz[b.nbr.long()]).sum(-2)
        want = (R @ (verts - xbar)[None, :, :, None])[..., 0] + xbar[None] + trans[:, :1]
    assert scale is None and float((xyz - want).abs().max()) < 1e-13
    sign = torch.where(qh[..., 3:] < 0, -1.0, 1.0).to(D)
    assert float((rot - sign * qh).abs().max()) < 1e-13


@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_identity_nodes_leave_the_vertices_unchanged(method):
    gen = torch.Generator().manual_seed(2)
    verts, node_xyz, b = _graph(gen)
    T, P = 3, b.n_nodes
    q = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=D).expand(T, P, 4).contiguous()
    w = b.w.double() / b.w.double().sum(-1, keepdim=True)  # (the float32 weights sum to 1 within 1e-7 only)
    xyz, rot, _ = ref.skin_vertices_reference(verts, node_xyz, torch.zeros(T, P, 3, dtype=D), q, b.nbr.long(), w,
                                              method)
    assert float((xyz - verts[None]).abs().max()) < 1e-14
    assert torch.equal(rot, q[:, :1].expand(T, b.n_verts, 4))


def test_identity_vertex_rotations_give_rotation0():
    v, f = gs.icosphere(1)
    faces = torch.tensor(f)
    mb = MeshBinding.from_reference_count(faces, len(v), 6)
    gen = torch.Generator().manual_seed(3)
    T, V, N = 2, len(v), mb.n_gaussians
    vx = torch.tensor(v, dtype=D)[None] + 0.05 * torch.randn(T, V, 3, generator=gen, dtype=D)
    vr = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=D).expand(T, V, 4)
    q0 = torch.nn.functional.normalize(torch.randn(N, 4, generator=gen, dtype=D), dim=-1)
    xyz, rotation, normals, scaling = ref.timed_gaussians_reference(vx, vr, q0, faces, mb.bary)
    assert scaling is None and float((rotation - q0[None]).abs().max()) < 1e-15
    assert float((normals.norm(dim=-1) - 1).abs().max()) < 1e-13
    # the barycentric points lie in their faces' planes (the float32 table's rows sum to 1 within 6e-8)
    fv = vx[:, faces]
    off = ((xyz.view(T, -1, 6, 3) - fv[:, :, None, 0]) * normals.view(T, -1, 6, 3)).sum(-1)
    assert float(off.abs().max()) < 1e-7
    # with scales: component 0 of vert_scale is discarded
    vs = torch.randn(T, V, 3, generator=gen, dtype=D)
    ls = torch.randn(N, 2, generator=gen, dtype=D)
    a = ref.timed_gaussians_reference(vx, vr, q0, faces, mb.bary, vs, ls, 1e-3)[3]
    vs2 = vs.clone()
    vs2[..., 0] += 5
    assert torch.equal(a, ref.timed_gaussians_reference(vx, vr, q0, faces, mb.bary, vs2, ls, 1e-3)[3])
    assert torch.equal(a[..., 0], torch.full((T, N), 1e-3, dtype=D))


@pytest.mark.parametrize("method", ["dqs", "lbs"])
def test_gradcheck_of_the_skinning_restatement(method):
    gen = torch.Generator().manual_seed(4)
    verts, node_xyz, b = _graph(gen, V=7, P=5, K=3)
    T, P = 2, 5
    q = random_quats(gen, (T, P), D, identity_every=4).requires_grad_()
    trans = torch.randn(T, P, 3, generator=gen, dtype=D).requires_grad_()
    scales = torch.randn(T, P, 3, generator=gen, dtype=D).requires_grad_()
    verts = verts.clone().requires_grad_()
    fn = lambda vv, tt, qq, ss: ref.skin_vertices_reference(vv, node_xyz, tt, qq, b.nbr.long(), b.w.double(), method,
                                                            ss)
    assert torch.autograd.gradcheck(fn, (verts, trans, q, scales), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_gradcheck_of_the_timed_restatement():
    gen = torch.Generator().manual_seed(5)
    v, f = gs.icosphere(0)
    faces = torch.tensor(f)[:6]
    bary = MeshBinding.from_reference_count(faces, 12, 3).bary.double()
    T, V, N = 2, 12, 18
    vx = (torch.tensor(v, dtype=D)[None] + 0.05 * torch.randn(T, V, 3, generator=gen, dtype=D)).requires_grad_()
    vr = random_quats(gen, (T, V), D, identity_every=5).requires_grad_()
    q0 = torch.randn(N, 4, generator=gen, dtype=D).requires_grad_()
    vs = (0.1 * torch.randn(T, V, 3, generator=gen, dtype=D)).requires_grad_()
    ls = (0.3 * torch.randn(N, 2, generator=gen, dtype=D)).requires_grad_()
    fn = lambda a, b, c, d, e: ref.timed_gaussians_reference(a, b, c, faces, bary, d, e, 1e-3)
    assert torch.autograd.gradcheck(fn, (vx, vr, q0, vs, ls), eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- SkinBinding --------------------------------------------------------------------------------------------------
def _check_incidence(b, nbr):
    flat = nbr.reshape(-1).long()
    V, K, P = b.n_verts, b.n_neighbors, b.n_nodes
    assert b.nbr.dtype == torch.int32 and torch.equal(b.nbr.long(), nbr.long())
    assert b.w.dtype == torch.float32 and b.w.shape == (V, K)
    assert b.item_order.dtype == torch.int32 and b.item_order.shape == (V * K,)
    assert b.node_offsets.dtype == torch.int32 and b.node_offsets.shape == (P + 1,)
    assert sorted(b.item_order.tolist()) == list(range(V * K))  # every item once
    for j in range(P):  # brute force: the items of node j, ascending
        want = [i for i in range(V * K) if int(flat[i]) == j]
        assert b.item_order[int(b.node_offsets[j]):int(b.node_offsets[j + 1])].tolist() == want, j


def test_skin_binding_incidence():
    nbr = torch.tensor([[0, 2], [2, 1], [2, 0], [4, 2]])
    w = torch.tensor([[0.25, 0.75], [0.5, 0.5], [1.0, 0.0], [0.1, 0.9]], dtype=torch.float64)
    b = SkinBinding(nbr, w, 5)  # node 3: no vertex
    assert (b.n_verts, b.n_nodes, b.n_neighbors) == (4, 5, 2)
    assert b.item_order.tolist() == [0, 5, 3, 1, 2, 4, 7, 6]
    assert b.node_offsets.tolist() == [0, 2, 3, 7, 7, 8]
    assert torch.equal(b.w, w.float())
    _check_incidence(b, nbr)
    gen = torch.Generator().manual_seed(6)
    big = torch.randint(0, 9, (40, 5), generator=gen)
    _check_incidence(SkinBinding(big.to(torch.int16), torch.rand(40, 5, generator=gen), 11), big)
    empty = SkinBinding(torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3), 2)
    assert empty.n_verts == 0 and empty.node_offsets.tolist() == [0, 0, 0] and empty.item_order.numel() == 0
    moved = b.to("cpu")
    assert moved is not b and torch.equal(moved.nbr, b.nbr) and torch.equal(moved.item_order, b.item_order)
    assert moved.device.type == "cpu"


def test_skin_binding_argument_errors():
    nbr = torch.tensor([[0, 2], [2, 1]])
    w = torch.full((2, 2), 0.5)
    bad = [
        (nbr.float(), w, 3), (nbr.tolist(), w, 3), (nbr.bool(), w, 3),  # not an integer tensor
        (nbr.reshape(-1), w.reshape(-1), 3), (nbr[None], w[None], 3),  # not (V, K)
        (torch.zeros(2, 0, dtype=torch.int64), torch.zeros(2, 0), 3),  # K = 0
        (torch.zeros(2, 33, dtype=torch.int64), torch.zeros(2, 33), 3),  # K = 33
        (nbr, w[:1], 3), (nbr, w.long(), 3), (nbr, w.tolist(), 3),  # weights
        (nbr, w, 2), (torch.tensor([[0, -1], [1, 1]]), w, 3),  # an entry out of range
        (nbr, w, -1), (nbr, w, 3.0), (nbr, w, True),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            SkinBinding(*args)
    assert SkinBinding(torch.zeros(2, 32, dtype=torch.int64), torch.zeros(2, 32), 1).n_neighbors == 32


def test_from_euclidean_against_brute_force():
    gen = torch.Generator().manual_seed(7)
    verts, nodes = torch.randn(50, 3, generator=gen), torch.randn(12, 3, generator=gen)
    b = SkinBinding.from_euclidean(verts, nodes, 4, chunk=16)  # several chunks
    dist, idx = torch.topk(torch.cdist(verts.double(), nodes.double()), 4, dim=1, largest=False)
    assert torch.equal(b.nbr.long(), idx)
    assert float((b.w.double() - dist / dist.sum(-1, keepdim=True)).abs().max()) < 1e-6
    assert float((b.w.double().sum(-1) - 1).abs().max()) < 1e-6
    assert (b.w[:, 1:] >= b.w[:, :-1]).all()  # the weight grows with the distance, as the reference has it
    _check_incidence(b, idx)
    for K in (0, 13, 33, 2.0, True):
        with pytest.raises(ValueError):
            SkinBinding.from_euclidean(verts, nodes, K)
    with pytest.raises(ValueError):
        SkinBinding.from_euclidean(verts[:, :2], nodes, 4)


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_skin_vertices_argument_errors():
    nbr = torch.tensor([[0, 2], [2, 1], [1, 1]])
    b = SkinBinding(nbr, torch.full((3, 2), 0.5), 4)
    ok = dict(verts=torch.zeros(3, 3), node_xyz=torch.zeros(4, 3), node_trans=torch.zeros(2, 4, 3),
              node_rots=torch.zeros(2, 4, 4), node_scales=None)
    bad = [
        dict(ok, verts=torch.zeros(4, 3)), dict(ok, verts=torch.zeros(3, 3, dtype=torch.float64)),
        dict(ok, verts=[[0.0] * 3] * 3), dict(ok, node_xyz=torch.zeros(5, 3)), dict(ok, node_xyz=torch.zeros(4, 2)),
        dict(ok, node_trans=torch.zeros(4, 3)), dict(ok, node_trans=torch.zeros(2, 5, 3)),
        dict(ok, node_trans=torch.zeros(2, 4, 3, dtype=torch.float16)),
        dict(ok, node_rots=torch.zeros(3, 4, 4)), dict(ok, node_rots=torch.zeros(2, 4, 3)),
        dict(ok, node_scales=torch.zeros(2, 4, 4)), dict(ok, node_scales=torch.zeros(1, 4, 3)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            skin_vertices(kw["verts"], kw["node_xyz"], kw["node_trans"], kw["node_rots"], b, "dqs", kw["node_scales"])
    args = (ok["verts"], ok["node_xyz"], ok["node_trans"], ok["node_rots"])
    with pytest.raises(ValueError, match="SkinBinding"):
        skin_vertices(*args, nbr)
    with pytest.raises(ValueError, match="method"):
        skin_vertices(*args, b, "slerp")
    for method in ("dqs", "lbs"):
        with pytest.raises(ValueError, match="no CPU path"):  # well-formed CPU tensors
            skin_vertices(*args, b, method)


def test_timed_gaussians_argument_errors():
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    b = MeshBinding.from_reference_count(faces, 4, 3)
    ok = dict(vert_xyz=torch.zeros(2, 4, 3), vert_rot=torch.zeros(2, 4, 4), rotation0=torch.zeros(6, 4))
    opt = dict(vert_scale=torch.zeros(2, 4, 3), log_scales=torch.zeros(6, 2), thickness=1e-3)
    bad = [
        dict(ok, vert_xyz=torch.zeros(4, 3)), dict(ok, vert_xyz=torch.zeros(2, 5, 3)),
        dict(ok, vert_xyz=torch.zeros(2, 4, 3, dtype=torch.float64)), dict(ok, vert_rot=torch.zeros(2, 4, 3)),
        dict(ok, vert_rot=torch.zeros(3, 4, 4)), dict(ok, rotation0=torch.zeros(5, 4)),
        dict(ok, rotation0=torch.zeros(6, 3)), dict(ok, rotation0=torch.zeros(6, 4, dtype=torch.float16)),
        dict(ok, **dict(opt, vert_scale=torch.zeros(2, 4, 2))), dict(ok, **dict(opt, log_scales=torch.zeros(6, 3))),
        dict(ok, **dict(opt, log_scales=torch.zeros(4, 2))), dict(ok, **dict(opt, thickness="thin")),
        dict(ok, vert_scale=opt["vert_scale"]), dict(ok, log_scales=opt["log_scales"], thickness=1e-3),
        dict(ok, thickness=1e-3),  # the optional inputs: all or none
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            timed_gaussians(kw.pop("vert_xyz"), kw.pop("vert_rot"), kw.pop("rotation0"), b, **kw)
    with pytest.raises(ValueError, match="F x G"):
        timed_gaussians(ok["vert_xyz"], ok["vert_rot"], torch.zeros(7, 4), b)
    with pytest.raises(ValueError, match="MeshBinding"):
        timed_gaussians(*ok.values(), faces)
    with pytest.raises(ValueError, match="no CPU path"):
        timed_gaussians(*ok.values(), b)
    with pytest.raises(ValueError, match="no CPU path"):
        timed_gaussians(*ok.values(), b, **opt)


def test_c_entries_check_their_arguments_without_gpu():
    lib = _C.load_library()
    assert lib.gsr_sugar_skin_workspace_bytes(0, 0, 0) > 0 and lib.gsr_sugar_timed_workspace_bytes(0, 0) > 0
    for T, V, P in ((1, 1, 1), (3, 200, 40), (8, 163_842, 1000)):
        want = 88 * T * P + 56 * T * V
        assert want <= lib.gsr_sugar_skin_workspace_bytes(T, V, P) <= want + 3 * 256
    for T, F in ((1, 1), (3, 1280), (8, 327_680)):
        assert 120 * T * F <= lib.gsr_sugar_timed_workspace_bytes(T, F) <= 120 * T * F + 256
    v = ctypes.c_void_p(16)  # never dereferenced: the calls fail validation first
    big = 1 << 40

    def skin(T, V, P, K, method, verts, nx, nt, nr, ns, nbr, w):
        return _C.SugarSkin(T=T, V=V, P=P, K=K, method=method, verts=verts, node_xyz=nx, node_trans=nt, node_rots=nr,
                            node_scales=ns, nbr=nbr, w=w)

    def sfwd(T=2, V=3, P=4, K=2, method=0, verts=v, nx=v, nt=v, nr=v, ns=None, nbr=v, w=v, xyz=v, rot=v, sc=None, ws=v,
             nbytes=big):
        return lib.gsr_sugar_skin_forward(skin(T, V, P, K, method, verts, nx, nt, nr, ns, nbr, w), xyz, rot, sc, ws,
                                          nbytes, None)

    def sbwd(T=2, V=3, P=4, K=2, method=0, verts=v, nx=v, nt=v, nr=v, ns=None, nbr=v, w=v, io=v, no=v, g=(v, v, None),
             dv=v, dt=v, dr=v, ds=None, ws=v, nbytes=big):
        return lib.gsr_sugar_skin_backward(skin(T, V, P, K, method, verts, nx, nt, nr, ns, nbr, w), io, no, *g, dv, dt,
                                           dr, ds, ws, nbytes, None)

    assert lib.gsr_sugar_skin_forward(None, v, v, None, v, big, None) == 1 and b"null" in lib.gsr_last_error()
    assert lib.gsr_sugar_skin_backward(None, v, v, v, v, None, v, v, v, None, v, big, None) == 1
    assert b"null" in lib.gsr_last_error()
    for call in (sfwd, sbwd):
        for K in (0, 33):
            assert call(K=K) == 1 and b"K must" in lib.gsr_last_error()
        assert call(method=2) == 1 and b"method" in lib.gsr_last_error()
        assert call(T=-1) == 1 and call(V=-1) == 1 and call(P=-1) == 1
        assert call(T=1 << 16, V=1 << 15) == 1 and b"2^31" in lib.gsr_last_error()
        assert call(V=1 << 27, K=16) == 1 and b"2^31" in lib.gsr_last_error()
        assert call(P=0) == 1 and b"without nodes" in lib.gsr_last_error()
        for name in ("verts", "nx", "nt", "nr", "nbr", "w", "ws"):
            assert call(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
        assert call(nr=ctypes.c_void_p(24)) == 1 and b"aligned" in lib.gsr_last_error()
        assert call(nbytes=lib.gsr_sugar_skin_workspace_bytes(2, 3, 4) - 1) == 1
        assert b"workspace" in lib.gsr_last_error()
        assert call(T=0) == 0 and call(V=0) == 0  # nothing to launch
        assert call(T=0, verts=None, nx=None, nt=None, nr=None, nbr=None, w=None) == 0
    for name in ("xyz", "rot"):
        assert sfwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert sfwd(ns=v, sc=None) == 1 and b"null" in lib.gsr_last_error()  # node_scales without vert_scale
    assert sfwd(rot=ctypes.c_void_p(24)) == 1 and b"aligned" in lib.gsr_last_error()
    for name in ("io", "no", "dv", "dt", "dr"):
        assert sbwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert sbwd(ns=v, ds=None) == 1 and b"null" in lib.gsr_last_error()
    assert sbwd(g=(v, ctypes.c_void_p(24), None)) == 1 and b"aligned" in lib.gsr_last_error()
    assert sbwd(dr=ctypes.c_void_p(24)) == 1 and b"aligned" in lib.gsr_last_error()

    bary = (ctypes.c_float * 24)(*([1 / 3] * 24))

    def timed(T, V, F, G, vx, vr, q0, faces, vs, ls):
        return _C.SugarTimed(T=T, V=V, F=F, G=G, vert_xyz=vx, vert_rot=vr, rotation0=q0, vert_scale=vs, log_scales=ls,
                             faces=faces, thickness=1e-3)

    def tfwd(T=2, V=4, F=2, G=3, N=6, vx=v, vr=v, q0=v, faces=v, bary=bary, vs=None, ls=None, xyz=v, rot=v, nrm=v,
             sc=None):
        return lib.gsr_sugar_timed_forward(timed(T, V, F, G, vx, vr, q0, faces, vs, ls), N, bary, xyz, rot, nrm, sc,
                                           None)

    def tbwd(T=2, V=4, F=2, G=3, N=6, vx=v, vr=v, q0=v, faces=v, bary=bary, vs=None, ls=None, co=v, vo=v,
             g=(v, v, v, None), dx=v, dr=v, dq0=v, dvs=None, dls=None, ws=v, nbytes=big):
        return lib.gsr_sugar_timed_backward(timed(T, V, F, G, vx, vr, q0, faces, vs, ls), N, bary, co, vo, *g, dx, dr,
                                            dq0, dvs, dls, ws, nbytes, None)

    assert lib.gsr_sugar_timed_forward(None, 6, bary, v, v, v, None, None) == 1 and b"null" in lib.gsr_last_error()
    assert lib.gsr_sugar_timed_backward(None, 6, bary, v, v, v, v, v, None, v, v, v, None, None, v, big, None) == 1
    assert b"null" in lib.gsr_last_error()
    for call in (tfwd, tbwd):
        assert call(N=7, vx=None, vr=None, q0=None, faces=None) == 1 and b"F x G" in lib.gsr_last_error()
        for G in (0, 9):
            assert call(G=G, N=2 * G) == 1 and b"G must" in lib.gsr_last_error()
        assert call(T=-1) == 1 and call(V=-1) == 1 and call(F=-1, N=-3) == 1
        assert call(T=1 << 12, F=1 << 18, N=3 << 18) == 1 and b"2^31" in lib.gsr_last_error()
        for name in ("vx", "vr", "q0", "faces", "bary"):
            assert call(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
        assert call(vs=v) == 1 and call(ls=v) == 1 and b"together" in lib.gsr_last_error()
        for name in ("vr", "q0"):
            assert call(**{name: ctypes.c_void_p(24)}) == 1 and b"aligned" in lib.gsr_last_error(), name
        assert call(vs=v, ls=ctypes.c_void_p(20)) == 1 and b"aligned" in lib.gsr_last_error()
        assert call(T=0) == 0 and call(F=0, N=0) == 0  # nothing to launch
        assert call(F=0, N=0, vx=None, vr=None, q0=None, faces=None) == 0
    for name in ("xyz", "rot", "nrm"):
        assert tfwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert tfwd(vs=v, ls=v, sc=None) == 1 and b"null" in lib.gsr_last_error()
    assert tfwd(rot=ctypes.c_void_p(24)) == 1 and b"aligned" in lib.gsr_last_error()
    for name in ("co", "vo", "dx", "dr", "dq0", "ws"):
        assert tbwd(**{name: None}) == 1 and b"null" in lib.gsr_last_error(), name
    assert tbwd(vs=v, ls=v, dvs=v, dls=None) == 1 and tbwd(vs=v, ls=v, dvs=None, dls=v) == 1
    assert tbwd(g=(v, ctypes.c_void_p(24), v, None)) == 1 and b"aligned" in lib.gsr_last_error()
    assert tbwd(dq0=ctypes.c_void_p(24)) == 1 and b"aligned" in lib.gsr_last_error()
    assert tbwd(vs=v, ls=v, dvs=v, dls=ctypes.c_void_p(20)) == 1 and b"aligned" in lib.gsr_last_error()
    assert tbwd(nbytes=lib.gsr_sugar_timed_workspace_bytes(2, 2) - 1) == 1 and b"workspace" in lib.gsr_last_error()

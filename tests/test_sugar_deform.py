"""The deformation network without a GPU: the torch restatement (tests/sugar_deform_reference.py) against the
reference's own DeformationNetwork (tests/golden/reference_deform.npz, made by tests/golden/make_golden_deform.py), the
tables of HexPlaneBinding, DeformationWeights and the argument checks of the C calls."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

import sugar_deform_reference as ref  # noqa: E402
from diff_gaussian_rasterization import _C  # noqa: E402
from sugar_deform_reference import CASES, fixture, fixture_reference, fixture_ups, fixture_weights  # noqa: E402

RESOLUTION, MULTIRES = (4, 5, 6, 3), (1, 2)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_reproduces_the_reference(case):
    z = fixture()
    normalize, d_scale = CASES[case]
    w = fixture_weights(z, d_scale)
    r64, r32 = (fixture_reference(z, case, tag, w) for tag in ("f64", "f32"))
    assert len(r64) == {"dg": 29, "dg_noscale": 11, "vert": 15}[case], len(r64)
    res = {dt: ref.evaluate(dt, z["points"], z["ticks"], z["aabb"], w.planes, w.mlp, fixture_ups(z, d_scale), normalize)
           for dt in (torch.float64, torch.float32)}
    for k, want in r64.items():
        assert want.dtype == torch.float64 and want.any(), k
        e64, e32, null = _rel(res[torch.float64][k], want), _rel(res[torch.float32][k], want), _rel(r32[k], want)
        print(f"{case} {k}: restatement f64 {e64:.3g}  f32 {e32:.3g}  reference f32 {null:.3g}")
        assert e64 <= 1e-12, (case, k, e64)
        assert e32 <= 2 * null, (case, k, e32, null)


def _binding(P=40, T=6, seed=0):
    from sugar_deform import HexPlaneBinding

    gen = torch.Generator().manual_seed(seed)
    points = torch.rand(P, 3, generator=gen) * 2.6 - 1.3  # some outside the box on both sides
    points[0] = torch.tensor([-1.0 / 3.0, 0.5, -0.2])  # y exactly on texel 1 of the first level's 5
    points[1] = -1.0  # the upper edge (n = +1)
    ticks = torch.linspace(-0.1, 1.1, T)
    aabb = torch.tensor([[1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])
    return HexPlaneBinding(points, ticks, aabb, RESOLUTION, MULTIRES), points, ticks, aabb


def test_binding_cells_match_the_restatement():
    b, points, ticks, aabb = _binding()
    n = ref.normalize_aabb(points.double(), aabb.double())
    for l, reso in enumerate(b.reso):
        for d in range(3):
            c = ((n[:, d] + 1) / 2 * (reso[d] - 1)).clamp(0, reso[d] - 1)
            assert torch.equal(b.cell[l, d].double() + b.frac[l, d], c)
            assert (b.frac[l, d] >= 0).all() and (b.frac[l, d] < 1).all()
    assert b.frac.dtype == torch.float64 and b.cell.dtype == torch.int32
    assert (b.cell[:, :, 1] == torch.tensor(b.reso)[:, :3] - 1).all() and not b.frac[:, :, 1].any()
    assert b.frac[0, 1, 0] == 0 and b.cell[0, 1, 0] == 1  # y = 0.5: n = -0.5, exactly texel 1 of 5


def test_binding_tables():
    """Each table is a permutation of the in-plane (point, corner) entries, and its row-wise gather equals a scatter."""
    from sugar_deform import COMBOS, SPATIAL_PLANES

    b, _, _, _ = _binding()
    P, T, L = b.P, b.T, b.L
    gen = torch.Generator().manual_seed(1)
    # spatial planes
    base, seen = 0, 0
    for l in range(L):
        for q in SPATIAL_PLANES:
            a, bb = COMBOS[q]
            Ra, Rb = b.reso[l][a], b.reso[l][bb]
            rows = b.sp_offsets[base:base + Ra * Rb + 1].long()
            order = b.sp_order[rows[0]:rows[-1]].long()
            e = torch.arange(4 * P)
            x, y = b.cell[l, a][e >> 2] + (e & 1), b.cell[l, bb][e >> 2] + ((e >> 1) & 1)
            inside = (x < Ra) & (y < Rb)
            assert sorted(order.tolist()) == e[inside].tolist()  # a permutation; out-of-plane corners absent
            assert not inside.all()  # (the upper-edge point has corners outside)
            val = torch.randn(4 * P, generator=gen, dtype=torch.float64)
            scatter = torch.zeros(Ra * Rb, dtype=torch.float64).index_add_(0, (y * Ra + x)[inside].long(), val[inside])
            gather = torch.stack([val[b.sp_order[rows[i]:rows[i + 1]].long()].sum() for i in range(Ra * Rb)])
            assert torch.allclose(scatter, gather, rtol=0, atol=1e-12)
            for i in range(Ra * Rb):
                r = b.sp_order[rows[i]:rows[i + 1]]
                assert (r[1:] > r[:-1]).all()  # ascending entries: the sum order
            base += Ra * Rb
            seen += int(inside.sum())
    assert base == b.n_sp_texels and seen == b.sp_order.numel() and b.sp_offsets.numel() == base + 1
    # columns
    base = 0
    for l in range(L):
        for d in range(3):
            R = b.reso[l][d]
            rows = b.col_offsets[base:base + R + 1].long()
            e = torch.arange(2 * P)
            x = b.cell[l, d][e >> 1] + (e & 1)
            assert sorted(b.col_order[rows[0]:rows[-1]].tolist()) == e[x < R].tolist()
            for i in range(R):
                assert (x[b.col_order[rows[i]:rows[i + 1]].long()] == i).all()
            base += R
    assert base == b.n_columns and b.col_offsets.numel() == base + 1
    e = torch.arange(2 * T)
    row = b.tcell[e >> 1] + (e & 1)
    assert sorted(b.t_order.tolist()) == e[row < b.reso[0][3]].tolist()
    for i in range(b.reso[0][3]):
        assert (row[b.t_order[b.t_offsets[i]:b.t_offsets[i + 1]].long()] == i).all()


def test_binding_size_formula():
    b, _, _, _ = _binding()
    P, T, L = b.P, b.T, b.L
    rows = b.n_sp_texels + b.n_columns + b.reso[0][3] + 3
    entries = b.sp_order.numel() + b.col_order.numel() + b.t_order.numel()
    assert b.nbytes == 36 * L * P + 12 * T + 4 * entries + 4 * rows
    assert b.sp_order.numel() <= 12 * L * P and b.col_order.numel() <= 6 * L * P and b.t_order.numel() <= 2 * T
    assert b.nbytes <= 108 * L * P + 20 * T + 4 * rows
    from sugar_deform import level_resolutions

    full = level_resolutions((64, 64, 64, 25), (1, 2, 4, 8))
    assert sum(r[0] * r[1] + r[0] * r[2] + r[1] * r[2] for r in full) == 1044480 and sum(sum(r[:3]) for r in full) == 2880
    assert b.to("cpu").nbytes == b.nbytes and b.device.type == "cpu"


def test_weights_round_trip_and_initialisation():
    from sugar_deform import DeformationWeights

    z = fixture()
    w = fixture_weights(z, True)
    assert sorted(w.names) == sorted(z["names"]) and w.L == 2 and w.reso == [[4, 5, 6, 3], [8, 10, 12, 3]]
    assert all(t.requires_grad and t.is_leaf for t in w.parameters())
    sd = w.state_dict()
    for k in z["names"]:
        assert torch.equal(sd[k].detach(), z["w_" + k]), k
    ignored = set(z["all_names"]) - set(z["names"])
    assert any("timenet" in k for k in ignored) and any("opacity_deform" in k for k in ignored)
    full = {k: (z["w_" + k] if "w_" + k in z else torch.zeros(1)) for k in z["all_names"]}
    assert DeformationWeights.from_state_dict(full, True).names == w.names
    assert len(DeformationWeights.from_state_dict(full, False).mlp) == 10
    with pytest.raises(ValueError):
        DeformationWeights.from_state_dict({k: v for k, v in full.items() if "pos_deform.feature_out.1.bias" not in k})
    init = DeformationWeights.init_like_reference(torch.Generator().manual_seed(0), RESOLUTION, MULTIRES)
    assert [tuple(t.shape) for t in init.parameters()] == [tuple(t.shape) for t in w.parameters()]
    for i, p in enumerate(t.detach() for t in init.planes):
        if i % 6 in (2, 4, 5):
            assert (p == 1).all()
        else:
            assert float(p.min()) >= 0.1 and float(p.max()) <= 0.5 and float(p.std()) > 0.05
    assert init.mlp[0].any() and float(init.mlp[0].abs().max()) <= (6.0 / (64 + 64)) ** 0.5
    assert not any(t.any() for t in init.mlp[2:])


def test_argument_errors_without_gpu():
    """Validation happens before any device work: nothing here is ever dereferenced on a device."""
    lib = _C.load_library()
    a = 16
    reso = (ctypes.c_int * 8)(4, 5, 6, 3, 8, 10, 12, 3)
    planes = (ctypes.c_void_p * 12)(*([a] * 12))
    mlp = (ctypes.c_void_p * 14)(*([a] * 14))

    def call(**fields):
        base = dict(T=2, P=3, L=2, d_scale=1, normalize_rot=1, reso=reso, planes=planes, mlp=mlp, cell=a, frac=a,
                    tcell=a, tfrac=a)
        c = _C.SugarDeform(**dict(base, **fields))
        rc = (lib.gsr_sugar_deform_forward(c, a, a, a, None),
              lib.gsr_sugar_deform_backward(c, a, a, a, a, a, a, a, a, a, planes, mlp, a, 1 << 40, None))
        assert rc == (1, 1), rc
        return lib.gsr_last_error()

    assert b"L must be in 1..4" in call(L=0)
    assert b"L must be in 1..4" in call(L=5)
    assert b"negative size" in call(T=-1)
    assert b"below 2^31" in call(T=1 << 16, P=1 << 16)
    assert b"at least 2" in call(reso=(ctypes.c_int * 8)(4, 5, 1, 3, 8, 10, 12, 3))
    assert b"time resolution" in call(reso=(ctypes.c_int * 8)(4, 5, 6, 3, 8, 10, 12, 4))
    holes = (ctypes.c_void_p * 12)(*([a] * 7 + [None] + [a] * 4))
    assert b"null plane" in call(planes=holes)
    assert b"null pointer" in call(planes=None)
    no_scale = (ctypes.c_void_p * 14)(*([a] * 10))
    assert b"scale head" in call(mlp=no_scale)
    assert b"scale head" in call(d_scale=0)
    assert b"8-byte aligned" in call(frac=20)
    c = _C.SugarDeform(T=2, P=3, L=2, d_scale=1, normalize_rot=1, reso=reso, planes=planes, mlp=mlp, cell=a, frac=a,
                       tcell=a, tfrac=a)
    assert lib.gsr_sugar_deform_forward(c, a, None, a, None) == 1
    assert lib.gsr_sugar_deform_backward(c, a, a, a, a, a, a, a, a, a, planes, mlp, a, 16, None) == 1
    assert b"workspace too small" in lib.gsr_last_error()
    assert lib.gsr_sugar_deform_workspace_bytes(32, 1000, 4) >= 8 * 128 * (32 * 1000 + 2 * 1000)
    assert lib.gsr_sugar_deform_workspace_bytes(0, 0, 4) > 0 and lib.gsr_sugar_deform_workspace_bytes(1, 1, 0) == 0
    empty = _C.SugarDeform(T=0, P=3, L=2, d_scale=1, normalize_rot=1, reso=reso, planes=planes, mlp=mlp)
    assert lib.gsr_sugar_deform_forward(empty, None, None, None, None) == 0  # launches nothing


def test_needs_a_gpu():
    from sugar_deform import DeformationWeights, deformation_knots

    b, _, _, _ = _binding()
    w = DeformationWeights.init_like_reference(None, RESOLUTION, MULTIRES)
    with pytest.raises(ValueError, match="no CPU path"):
        deformation_knots(b, w)

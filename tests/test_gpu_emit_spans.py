"""The emission's span-word gather (csrc/gsr_binning.hip k_emit<false, true>, csrc/gsr_span_word.h) against the record
path (GSR_EMIT_SPANS=0: k_emit<false, false>, every Gaussian's rows from span_prep / span_row), bitwise: all rendered
outputs and radii, every parameter gradient and per-view means2D gradient, and the num_rendered / listed-instance
counts the Python layer records.  The switch is read once per process, so one child process runs every case with the
other setting (tests/emit_span_cases.py run_all) and each test compares its case.  Each test first asserts on the CPU
(emit_span_cases.spans_cpu: the oracle's fp32 preprocess values through span_prep / span_row restated in float32)
that its scene really holds the case it names."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emit_span_cases as ec

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def other(tmp_path_factory):
    """Every case under the other setting of GSR_EMIT_SPANS than this process has, from one child process."""
    out = tmp_path_factory.mktemp("emit_spans") / "other.npz"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    if env.pop("GSR_EMIT_SPANS", None) != "0":
        env["GSR_EMIT_SPANS"] = "0"
    code = "import emit_span_cases as ec; ec.run_all(%r)" % str(out)
    res = subprocess.run([sys.executable, "-c", code], cwd=HERE, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    return np.load(out)


def assert_same(name, mine, other):
    keys = sorted(k for k in other.files if k.startswith(name + "__"))
    assert len(keys) == len(mine) and len(mine) > 6
    for k, x in zip(keys, mine):
        y = other[k]
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True), \
            f"{name}: array {k} differs between the span-word and the record emission"


def views(name):
    scene, cams = ec.case(name)
    return [ec.spans_cpu(scene, cam) for cam in cams]


def chunk_kept(sp, g):
    """Kept positions of each 64-row chunk of group g's row list (the emission's k0 loop runs past 64 of them)."""
    ln = np.concatenate([sp["len"][i, :sp["rows"][i]] for i in g]) if len(g) else np.zeros(0, np.int64)
    return [int(ln[i:i + 64].sum()) for i in range(0, len(ln), 64)]


def test_ball_mostly_encodable(other):
    sps = views("ball")
    for sp in sps:
        assert sp["enc"].sum() > 0.9 * sp["vis"].sum() > 0
    # encodable lanes through both chunk loops: a group of more than 64 rows, a row chunk of more than 64 kept tiles
    sp = sps[0]
    assert any(sp["rows"][g].sum() > 64 and max(chunk_kept(sp, g)) > 64 for g in ec.groups(sp) if sp["enc"][g].all())
    assert_same("ball", ec.run_case("ball"), other)


def test_limits_mixed_in_one_wave(other):
    """Exactly 4 (encodable) and exactly 5 rectangle rows, rows of exactly 15 (encodable) and 16 kept tiles, in one
    64-Gaussian group of the depth order, and in one 64-row chunk of it."""
    found = chunk = 0
    for sp in views("mixed"):
        rows, ln, enc = sp["rows"], sp["len"], sp["enc"]
        for g in ec.groups(sp):
            r4 = (rows[g] == 4) & enc[g]
            r5 = rows[g] == 5
            l15 = (ln[g].max(1) == 15) & enc[g]
            l16 = ln[g].max(1) == 16
            if r4.any() and r5.any() and l15.any() and l16.any():
                found += 1
                # consecutive Gaussians of the group, one encodable and one not, share a row chunk
                e = enc[g]
                first_row = np.cumsum(rows[g]) - rows[g]
                chunk += int(any(e[i] != e[i + 1] and first_row[i] // 64 == first_row[i + 1] // 64
                                 for i in range(len(g) - 1)))
        assert not enc[(rows == 5) | (ln.max(1) == 16)].any()
    assert found > 0 and chunk > 0
    assert_same("mixed", ec.run_case("mixed"), other)


def test_tile_column_128(other):
    """2064 x 32: 129 tile columns; kept spans end below, at and past column 127."""
    for sp in views("wide"):
        assert sp["rect"][:, 2].max() == 129
        last = sp["t1"].max(1)  # one past the last kept column
        has = sp["len"].sum(1) > 0
        assert (sp["enc"] & has & (last <= 120)).any() and (sp["enc"] & has & (last == 128)).any()
        assert (~sp["enc"] & sp["vis"] & (last == 129)).any() and (sp["vis"] & (sp["t0"].max(1) == 128)).any()
        assert not sp["enc"][last > 128].any()
    assert_same("wide", ec.run_case("wide"), other)


def test_empty_rows(other):
    """Rectangles none of whose rows keeps a tile (opacity below 1/255), and rectangles whose first or last rows
    keep none while others do.  An empty row between two kept ones does not occur: the kept region is an ellipse
    (convex), so the row bands it meets are consecutive, and span_row's margins only widen each band's extent."""
    for sp in views("faint"):
        ln, rows, enc = sp["len"], sp["rows"], sp["enc"]
        assert (enc & (ln.sum(1) == 0) & (rows >= 2)).sum() >= 100
        some = enc & (ln.sum(1) > 0)
        assert (some & (ln[:, 0] == 0)).any()
        last = ln[np.arange(len(rows)), np.maximum(rows - 1, 0)]
        assert (some & (last == 0)).any()
        for i in np.nonzero(sp["vis"])[0]:
            nz = np.nonzero(ln[i, :rows[i]])[0]
            assert len(nz) == 0 or nz[-1] - nz[0] + 1 == len(nz)  # (no empty middle row)
    assert_same("faint", ec.run_case("faint"), other)


def test_long_groups_and_chunks(other):
    """Groups of more than 64 rows (the r0 loop) and row chunks of more than 64 kept tiles (the k0 loop), with lanes
    of both kinds in them."""
    ok = 0
    for sp in views("long"):
        for g in ec.groups(sp):
            e = sp["enc"][g]
            if sp["rows"][g].sum() > 128 and max(chunk_kept(sp, g)) > 128 and e.any() and not e.all():
                ok += 1
    assert ok > 0
    assert_same("long", ec.run_case("long"), other)


def test_ragged_count_and_culled(other):
    scene, cams = ec.case("ragged")
    P = scene["means3D"].shape[0]
    assert P % 64 != 0 and P % 128 != 0
    sps = [ec.spans_cpu(scene, c) for c in cams]
    assert sps[0]["vis"].all()
    for sp in sps[1:]:
        assert 0 < sp["vis"].sum() < P and sp["vis"].sum() % 64 != 0
        assert sp["enc"].any() and (sp["vis"] & ~sp["enc"]).any()
    assert_same("ragged", ec.run_case("ragged"), other)


@pytest.mark.parametrize("name", ["timed", "two_colour"])
def test_other_producers(name, other):
    """A rasterize_timed_views call (k_preprocess_timed writes the words too) and a two-colour call."""
    assert_same(name, ec.RUNNERS[name](), other)

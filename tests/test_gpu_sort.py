"""The view-segmented stable radix sort (csrc/gsr_sort.hip; every sort of the library: depth, tile and Morton keys)
through its C-ABI entry gsr_sort_pairs, against numpy's stable sort (the scatter's per-wave running
counts are read by every lane and advanced by each digit's first lane — many equal digits per wave, ragged segment
tails, empty and one-item segments, full 4096-item blocks and bounded last blocks, keys-only and key/value, 4-, 6-
and 8-bit digits and the runtime-width path).  Bit-exact: integer work.

Sizes.  SEGS (the first tests): 11 segments, 57 k items, at most 5 blocks of 4096 in a segment, 16 blocks in all.
The tests after them reach the three regimes that list leaves out:
  - scan chunk carry (k_seg_scan walks a (segment, digit) row in chunks of 1024 block counts): one segment of
    4 194 304 (1024 full blocks, one chunk), 4 194 305 (1025 blocks: a second chunk of one block of one item) and
    8 388 609 items (2049 blocks: the carry is carried twice), with 3 and with 2^20 distinct keys;
  - row layout R * blk[v] + d * nb + lb at 64 segments (SEGS64_A / SEGS64_B: empty segments first, last and in
    adjacent pairs, 1-item segments, 4095 / 4096 / 4097, 4 194 305 items at index 31, 12 289 at the end) with
    (13, 5), (20, 7) (runtime-width last pass: R changes between passes) and (32, 8);
  - block map xcd_block(b, gridDim): total block counts 1, 2, 7, 8, 9, 15, 16, 17, 23 and 1025 .. 1032 (every
    residue mod 8 below and above a scan chunk), three segments each, ragged last block;
  - keys 0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF in runs and shuffled at 32, 31 and 1 key bits;
  - 4 KB guard tails behind keys, values and work buffer (even and odd pass counts).
test_model_* (no GPU) restate one pass of gsr_sort.hip in numpy at 4 194 305 items and show that these sizes tell
a dropped carry, a wrong row base and a block map that is no bijection from the right sort."""
import numpy as np
import pytest

from gsr_testutil import gpu_sort_pairs as _sort
from gsr_testutil import gpu_sort_pairs_guarded as _sort_guarded

gpu = pytest.mark.gpu  # (per test: the CPU model at the end of the module runs without a GPU)

SEGS = [0, 1, 63, 64, 4095, 4096, 4097, 12288, 20000 + 37, 0, 5]


def _expect(keys, vals, sizes, key_bits):
    mask = np.uint32(0xFFFFFFFF) if key_bits == 32 else np.uint32((1 << key_bits) - 1)
    ek, ev, o = keys.copy(), (vals.copy() if vals is not None else None), 0
    for n in sizes:
        seg = keys[o:o + n]
        order = np.argsort(seg & mask, kind="stable")
        ek[o:o + n] = seg[order]
        if vals is not None:
            ev[o:o + n] = vals[o:o + n][order]
        o += n
    return ek, ev


@gpu
@pytest.mark.parametrize("key_bits,max_bits", [(32, 8), (12, 6), (30, 8), (8, 4), (13, 5), (20, 7)])
@pytest.mark.parametrize("distinct", [3, 64, 1 << 20])
@pytest.mark.parametrize("with_vals", [True, False])
def test_sort_pairs_matches_stable_sort(key_bits, max_bits, distinct, with_vals):
    rng = np.random.default_rng(key_bits * 1000 + max_bits * 10 + distinct % 97)
    total = sum(SEGS)
    # few distinct keys: long runs of equal digits in every wave and round (the running-count path); high bits above
    # key_bits set at random (ignored by the sort, carried along)
    keys = rng.integers(0, distinct, size=total, dtype=np.uint64).astype(np.uint32)
    if key_bits < 32:
        keys = (keys & np.uint32((1 << key_bits) - 1)) | (rng.integers(0, 2, size=total, dtype=np.uint32)
                                                         << np.uint32(key_bits))
    vals = np.arange(total, dtype=np.uint32) if with_vals else None
    gk, gv = _sort(keys, vals, SEGS, key_bits, max_bits)
    ek, ev = _expect(keys, vals, SEGS, key_bits)
    np.testing.assert_array_equal(gk, ek)
    if with_vals:
        np.testing.assert_array_equal(gv, ev)  # stability: equal keys keep their input order


@gpu
def test_sort_pairs_all_equal_and_descending():
    """One digit for a whole segment (every lane of every round a peer of every other), and reversed input."""
    sizes = [4096 * 3 + 17, 8191]
    keys = np.concatenate([np.full(sizes[0], 0xABCDEF12, np.uint32),
                           np.arange(sizes[1], 0, -1, dtype=np.uint32)])
    vals = np.arange(sum(sizes), dtype=np.uint32)
    gk, gv = _sort(keys, vals, sizes, 32, 8)
    ek, ev = _expect(keys, vals, sizes, 32)
    np.testing.assert_array_equal(gk, ek)
    np.testing.assert_array_equal(gv, ev)


@gpu
def test_rank_mode_probe_selects_lds_atomics():
    """The scatter ranks equal digits with LDS atomic adds only after the once-per-process probe found the device
    servicing same-counter lanes in lane order (gsr_sort.hip k_lds_rank_probe); on MI355X it does, so the fast
    path is the one the other tests here check against numpy's stable sort."""
    from diff_gaussian_rasterization import _C

    assert _C.load_library().gsr_sort_rank_mode() == 1


@gpu
def test_ballot_ranks_give_the_same_bits(tmp_path):
    """GSR_SORT_RANK=ballot (read once per process: a child process) sorts to the same bits as the default."""
    import os
    import subprocess
    import sys

    rng = np.random.default_rng(7)
    sizes = [4096 * 2 + 5, 777, 12288]
    keys = rng.integers(0, 64, size=sum(sizes), dtype=np.uint64).astype(np.uint32)
    vals = np.arange(sum(sizes), dtype=np.uint32)
    np.save(tmp_path / "k.npy", keys)
    np.save(tmp_path / "v.npy", vals)
    code = (
        "import sys, numpy as np; sys.path[:0] = [%r, %r]; import gsr_testutil as t; from diff_gaussian_rasterization "
        "import _C; k = np.load(%r); v = np.load(%r); gk, gv = t.gpu_sort_pairs(k, v, %r, 32, 6); "
        "np.save(%r, gk); np.save(%r, gv); print(_C.load_library().gsr_sort_rank_mode())"
        % (os.path.dirname(os.path.abspath(__file__)),
           os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "threestudio-3dgs_amd"),
           str(tmp_path / "k.npy"), str(tmp_path / "v.npy"), sizes,
           str(tmp_path / "bk.npy"), str(tmp_path / "bv.npy")))
    env = dict(os.environ, GSR_SORT_RANK="ballot")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "0"  # the child ranked by ballot matching
    gk, gv = _sort(keys, vals, sizes, 32, 6)
    np.testing.assert_array_equal(gk, np.load(tmp_path / "bk.npy"))
    np.testing.assert_array_equal(gv, np.load(tmp_path / "bv.npy"))


# ---- the regimes SEGS does not reach: scan chunks, 64 unequal segments, grid residues, key edges, bounds ---------
TILE = 4096  # GSR_SORT_TILE
CHUNK = 1024  # block counts per iteration of k_seg_scan (256 threads x 4 entries)
N_ONE_CHUNK, N_TWO_CHUNKS, N_THREE_CHUNKS = CHUNK * TILE, CHUNK * TILE + 1, 2 * CHUNK * TILE + 1
MIXED = "mixed"  # half the items from 3 keys, half from 2^20


def _digit_plan(key_bits, max_bits):
    """(passes, bits) of gsr_common.h digit_plan."""
    passes = -(-key_bits // max_bits)
    return passes, -(-key_bits // passes)


def _keys(rng, total, distinct, key_bits):
    """`distinct` key values spread over all key_bits bits (so every pass sees them), MIXED: half the items from 3
    values and half from 2^20; the bits above key_bits are random (ignored by the sort, carried along)."""
    if distinct == MIXED:
        k = np.where(rng.integers(0, 2, size=total) == 0, rng.integers(0, 3, size=total),
                     rng.integers(3, 3 + (1 << 20), size=total)).astype(np.uint64)
    else:
        k = rng.integers(0, distinct, size=total, dtype=np.uint64)
    keys = (((k + 1) * 0x9E3779B1) & 0xFFFFFFFF).astype(np.uint32)  # (odd multiplier: distinct stays distinct)
    if key_bits < 32:
        keys = (keys >> np.uint32(32 - key_bits)) | (rng.integers(0, 1 << (32 - key_bits), size=total, dtype=np.uint64)
                                                     .astype(np.uint32) << np.uint32(key_bits))
    return keys


def _first_wrong_pass(keys, vals, sizes, key_bits, max_bits):
    """The first digit pass whose result is wrong: a key of p * bits bits is sorted by the same first p passes."""
    passes, bits = _digit_plan(key_bits, max_bits)
    for p in range(1, passes):
        gk, gv = _sort(keys, vals, sizes, p * bits, bits)
        ek, ev = _expect(keys, vals, sizes, p * bits)
        if not (np.array_equal(gk, ek) and (vals is None or np.array_equal(gv, ev))):
            return p - 1
    return passes - 1


def _check(keys, vals, sizes, key_bits, max_bits, got=None):
    """Bit-exact against the stable sort per segment; a mismatch is reported by position, segment, block, chunk and
    digit pass."""
    gk, gv = got if got is not None else _sort(keys, vals, sizes, key_bits, max_bits)
    ek, ev = _expect(keys, vals, sizes, key_bits)
    bad = gk != ek
    if vals is not None:
        bad |= gv != ev
    if not bad.any():
        return
    p = int(np.flatnonzero(bad)[0])
    start = np.concatenate([[0], np.cumsum(sizes)])
    v = int(np.searchsorted(start, p, side="right")) - 1
    lb = (p - int(start[v])) // TILE
    passes, bits = _digit_plan(key_bits, max_bits)
    pytest.fail(
        "%d of %d items differ from the stable sort; first at position %d = segment %d (%d items, %d blocks) item %d, "
        "block %d (%s the first 1024-block scan chunk): key %#x for %#x%s; first wrong digit pass %d of %d x %d bits"
        % (int(bad.sum()), bad.size, p, v, sizes[v], -(-sizes[v] // TILE), p - int(start[v]), lb,
           "past" if lb >= CHUNK else "within", int(gk[p]), int(ek[p]),
           "" if vals is None else ", value %d for %d" % (int(gv[p]), int(ev[p])),
           _first_wrong_pass(keys, vals, sizes, key_bits, max_bits), passes, bits))


@gpu
@pytest.mark.parametrize("distinct", [3, 1 << 20])
@pytest.mark.parametrize("key_bits,max_bits,with_vals", [(32, 8, True), (12, 6, False)])  # the renderer's two shapes
@pytest.mark.parametrize("n", [N_ONE_CHUNK, N_TWO_CHUNKS, N_THREE_CHUNKS])
def test_scan_chunk_boundary(n, key_bits, max_bits, with_vals, distinct):
    """One segment of 1024, 1025 and 2049 blocks: k_seg_scan's loop over chunks of 1024 block counts runs once, twice
    (the second chunk one block of one item) and three times.  3 distinct keys put every block's 4096 items into
    the same few rows, so the carry reaches millions and a dropped or doubled one moves whole blocks."""
    rng = np.random.default_rng(n % 1000 + key_bits + distinct % 97)
    keys = _keys(rng, n, distinct, key_bits)
    vals = np.arange(n, dtype=np.uint32) if with_vals else None
    _check(keys, vals, [n], key_bits, max_bits)


def _segs64(last_empty):
    s = [0, 1, 4095, 4096, 4097, 0, 0, 1, 63, 64, 65, 12288, 8191, 8193, 1, 0,  # 0 .. 15 (5, 6: an empty pair)
         777, 4096, 20037, 2, 4095, 4097, 1000, 1, 12287, 3, 8192, 5, 0, 0, 1,  # 16 .. 30 (28, 29: an empty pair)
         N_TWO_CHUNKS,  # 31: 1025 blocks, its rows cross a scan chunk
         1, 4097, 0, 9000, 4096, 1, 33, 16385, 0, 0, 4095, 2, 4096, 1, 5000, 0,  # 32 .. 47 (40, 41: an empty pair)
         1, 12289, 64, 4097, 1, 0, 8190, 31, 4096, 1, 3000, 4095, 7, 1]  # 48 .. 61
    s += [12289, 0] if last_empty else [0, 12289]
    assert len(s) == 64 and s[31] == N_TWO_CHUNKS
    return s


# GSR_SET_MAX segments of unequal block counts.  "An empty segment last" and "12 289 items at index 63" cannot hold
# in one list of 64: A ends ..., 0, 12289 and B ends ..., 12289, 0.
SEGS64_A, SEGS64_B = _segs64(False), _segs64(True)


@gpu
@pytest.mark.parametrize("key_bits,max_bits", [(13, 5), (20, 7), (32, 8)])  # digits 5+5+3, 7+7+6, 4 x 8
@pytest.mark.parametrize("segs", [SEGS64_A, SEGS64_B], ids=["tail63", "empty63"])
def test_64_unequal_segments(segs, key_bits, max_bits):
    """Row base R * blk[v] (R = 8 after 32 and 64 after 128 in the last pass), nb per segment and seg_of_block over
    equal blk[] neighbours, together with the chunk carry of segment 31."""
    rng = np.random.default_rng(64 + key_bits)
    total = sum(segs)
    keys = _keys(rng, total, MIXED, key_bits)
    _check(keys, np.arange(total, dtype=np.uint32), segs, key_bits, max_bits)


GRID_BLOCKS = [1, 2, 7, 8, 9, 15, 16, 17, 23] + [1025 + r for r in range(8)]


def _residue_sizes(blocks):
    """Three segments of `blocks` blocks in all: full blocks, a last block of one item, a last block of 777."""
    a = blocks // 3
    b = (blocks - a) // 2
    c = blocks - a - b
    sizes = [a * TILE, (b - 1) * TILE + 1 if b else 0, (c - 1) * TILE + 777]
    assert sum(-(-n // TILE) for n in sizes) == blocks
    return sizes


def _assert_untouched(touched):
    assert touched == [], "the sort wrote behind the stated size of: %s" % ", ".join(touched)


@gpu
@pytest.mark.parametrize("blocks", GRID_BLOCKS)
def test_grid_residues_and_bounds(blocks):
    """xcd_block(b, gridDim) is another permutation for every gridDim mod 8 (and gridDim >> 3 = 0, 1, 2, 128, 129);
    the same call runs with guard tails behind keys, values and work buffer, which must come back untouched."""
    sizes = _residue_sizes(blocks)
    rng = np.random.default_rng(blocks)
    total = sum(sizes)
    keys = rng.integers(0, 1 << 32, size=total, dtype=np.uint64).astype(np.uint32)
    vals = np.arange(total, dtype=np.uint32)
    gk, gv, touched = _sort_guarded(keys, vals, sizes, 32, 8)
    _check(keys, vals, sizes, 32, 8, got=(gk, gv))
    _assert_untouched(touched)


@gpu
@pytest.mark.parametrize("key_bits,max_bits", [(20, 7), (32, 8)], ids=["3-passes-copied-back", "4-passes-in-place"])
def test_bounds_across_a_scan_chunk(key_bits, max_bits):
    """Guard tails at 1025 blocks: an odd pass count leaves the result in the work buffer and gsr_sort_pairs copies
    it back (the renderer's (32, 8) and (12, 6) are both even, so (20, 7) stands in), an even one ends in place."""
    assert _digit_plan(key_bits, max_bits)[0] % 2 == (1 if key_bits == 20 else 0)
    rng = np.random.default_rng(5 + key_bits)
    keys = _keys(rng, N_TWO_CHUNKS, MIXED, key_bits)
    vals = np.arange(N_TWO_CHUNKS, dtype=np.uint32)
    gk, gv, touched = _sort_guarded(keys, vals, [N_TWO_CHUNKS], key_bits, max_bits)
    _check(keys, vals, [N_TWO_CHUNKS], key_bits, max_bits, got=(gk, gv))
    _assert_untouched(touched)


EDGE_KEYS = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)


@gpu
@pytest.mark.parametrize("key_bits,max_bits", [(32, 8), (31, 8), (1, 1)])
@pytest.mark.parametrize("shuffled", [False, True], ids=["runs", "shuffled"])
def test_key_edges(shuffled, key_bits, max_bits):
    """The smallest and largest keys and both sides of the sign bit, 3 blocks.  seg_key passes 0xFFFFFFFF through
    unrebased: it sorts last and stably; at 31 bits and 1 bit the high bits are carried along."""
    n = 2 * TILE + 1234
    rng = np.random.default_rng(4)
    if shuffled:
        keys = EDGE_KEYS[rng.integers(0, EDGE_KEYS.size, size=n)]
    else:  # runs of 200 .. 1200 equal keys (longer than a wave's 1024 items, across blocks), largest first
        runs = rng.integers(200, 1200, size=64)
        keys = np.repeat(EDGE_KEYS[::-1][np.arange(64) % EDGE_KEYS.size], runs)[:n]
    assert keys.size == n and np.unique(keys).size == EDGE_KEYS.size
    _check(keys, np.arange(n, dtype=np.uint32), [n], key_bits, max_bits)


# ---- a numpy model of one pass of gsr_sort.hip (no GPU): do the sizes above bind? --------------------------------
M32 = 0xFFFFFFFF
STALE = 0xA5A5A5A5  # what a count row nobody wrote holds (the work buffer is not cleared)
UNWRITTEN = np.uint32(0xDEADBEEF)


def _xcd_block(b, n):
    """gsr_common.h xcd_block: logical block of workgroup b of n."""
    x, q, r = b & 7, n >> 3, n & 7
    return x * q + np.minimum(x, r) + (b >> 3)


def _xcd_block_no_remainder(b, n):
    """A wrong block map: right when 8 divides n, otherwise it visits some blocks twice and others never."""
    return (b & 7) * (n >> 3) + (b >> 3)


def _identity(b, n):
    return b


class _PassModel:
    """count, scan and scatter of gsr_sort.hip for the digit (key >> shift) & (2^bits - 1) over segments `sizes`.
    What no fault below touches is computed once: the segments' blocks (seg_fill_blocks), each block's digit
    histogram (k_seg_count's LDS histogram) and each item's stable rank among its block's equal digits
    (k_seg_scatter's ranking)."""

    def __init__(self, keys, vals, sizes, shift, bits):
        self.keys, self.vals, self.R = keys, vals, 1 << bits
        sizes = np.asarray(sizes, np.int64)
        self.V = sizes.size
        self.start = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        self.blk = np.concatenate([[0], np.cumsum(-(-sizes // TILE))])
        self.nb = np.diff(self.blk)
        self.grid = int(self.blk[-1])
        self.seg = np.repeat(np.arange(self.V), sizes)
        self.lb = (np.arange(keys.size) - self.start[self.seg]) // TILE
        self.block = self.blk[self.seg] + self.lb  # each item's logical block
        self.digit = ((keys >> np.uint32(shift)) & np.uint32(self.R - 1)).astype(np.int64)
        self.hist = np.bincount(self.block * self.R + self.digit, minlength=self.grid * self.R)
        self.hist = self.hist.reshape(self.grid, self.R)
        self.rank = np.empty(keys.size, np.int64)
        digit8 = self.digit.astype(np.uint8)
        for d in np.flatnonzero(self.hist.sum(0)):
            at = np.flatnonzero(digit8 == d)
            b = self.block[at]  # (ascending: items are in index order)
            self.rank[at] = np.arange(at.size) - np.searchsorted(b, b, side="left")

    def seg_of_block(self, b):
        """gsr_common.h seg_of_block: the last v < V with blk[v] <= b, and the block within it."""
        v = np.searchsorted(self.blk[:-1], b, side="right") - 1
        return v, b - self.blk[v]

    def run(self, add_carry=True, R_count=None, R_scan=None, R_scatter=None, map_count=_xcd_block,
            map_scatter=_xcd_block):
        R, grid = self.R, self.grid
        Rc, Rs, Rt = (R if x is None else x for x in (R_count, R_scan, R_scatter))
        counts = np.full(256 * grid, STALE, np.int64)  # GSR_RADIX x blocks, as SortWork carves it
        # k_seg_count: workgroup b takes logical block map(b, grid) and writes its R counts at R blk[v] + d nb + lb
        blocks = np.unique(map_count(np.arange(grid), grid))
        v, lb = self.seg_of_block(blocks)
        rows = Rc * self.blk[v][:, None] + np.arange(R)[None, :] * self.nb[v][:, None] + lb[:, None]
        counts[rows] = self.hist[blocks]
        # k_seg_scan: one workgroup per (v, d) row, exclusive scan in chunks of 1024 entries with a running carry
        totals = np.zeros((self.V, 256), np.int64)
        for v in np.flatnonzero(self.nb):
            nb = int(self.nb[v])
            rows = counts[Rs * self.blk[v]:Rs * self.blk[v] + R * nb].reshape(R, nb)  # (a view: scanned in place)
            carry = np.zeros(R, np.int64)
            for c0 in range(0, nb, CHUNK):
                c = rows[:, c0:c0 + CHUNK].copy()
                inclusive = np.cumsum(c, axis=1)
                rows[:, c0:c0 + CHUNK] = ((carry[:, None] if add_carry else 0) + inclusive - c) & M32
                carry = (carry + inclusive[:, -1]) & M32
            totals[v, :R] = carry
        # k_seg_scatter: position in the segment = scan(totals)[d] + scanned count of (d, block) + rank in the block
        done = np.zeros(grid, bool)
        done[np.unique(map_scatter(np.arange(grid), grid))] = True
        dstart = (np.cumsum(totals, axis=1) - totals) & M32
        dcnt = counts[Rt * self.blk[self.seg] + self.digit * self.nb[self.seg] + self.lb]
        dst = self.start[self.seg] + ((dstart[self.seg, self.digit] + dcnt + self.rank) & M32)
        put = done[self.block] & (dst < self.keys.size)  # (a store outside the arrays is not modelled: left out)
        out_k = np.full(self.keys.size, UNWRITTEN, np.uint32)
        out_v = np.full(self.keys.size, UNWRITTEN, np.uint32)
        out_k[dst[put]] = self.keys[put]
        out_v[dst[put]] = self.vals[put]
        return out_k, out_v


MODEL_SIZES = [TILE + 1, N_TWO_CHUNKS]  # (a segment in front: the large one's row base is R * 2, not 0)


@pytest.fixture(scope="module")
def model():
    rng = np.random.default_rng(6)
    total = sum(MODEL_SIZES)
    keys = _keys(rng, total, MIXED, 8)
    vals = np.arange(total, dtype=np.uint32)
    return _PassModel(keys, vals, MODEL_SIZES, 0, 8), _expect(keys, vals, MODEL_SIZES, 8)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_model_equals_stable_sort(model):
    m, want = model
    assert m.grid == 1027 and m.nb[1] == CHUNK + 1
    assert _same(m.run(), want)


def test_model_without_the_chunk_carry_differs(model):
    """`off = carry + ...` without the carry: the totals stay right, the block past the first chunk lands on block
    0's places.  One item fewer (1024 blocks, one chunk) and the same fault sorts right."""
    m, want = model
    assert not _same(m.run(add_carry=False), want)
    rng = np.random.default_rng(7)
    sizes = [TILE + 1, N_ONE_CHUNK]
    keys = _keys(rng, sum(sizes), MIXED, 8)
    vals = np.arange(sum(sizes), dtype=np.uint32)
    assert _same(_PassModel(keys, vals, sizes, 0, 8).run(add_carry=False), _expect(keys, vals, sizes, 8))


@pytest.mark.parametrize("where", ["R_count", "R_scan", "R_scatter"])
def test_model_with_a_wrong_row_base_differs(model, where):
    """One of the three kernels takes the row base with the R of another pass (64 for 256)."""
    m, want = model
    assert not _same(m.run(**{where: 64}), want)


def test_model_block_map(model):
    """What binds xcd_block is that it is a bijection of [0, gridDim) for every gridDim mod 8.  The identity in only
    one of count and scatter is another bijection: every logical block is still counted once and scattered once, and
    everything is addressed by the logical block, so the result cannot change (the map is "speed only", gsr_common.h)
    — asserted here as it is.  A map that is right only when 8 divides the grid differs at every other grid size:
    the residues of test_grid_residues_and_bounds."""
    m, want = model
    for n in GRID_BLOCKS + [m.grid, 1626]:
        assert np.array_equal(np.sort(_xcd_block(np.arange(n), n)), np.arange(n)), n
    assert _same(m.run(map_count=_identity), want)
    assert _same(m.run(map_scatter=_identity), want)
    assert m.grid % 8 == 3
    assert not _same(m.run(map_count=_xcd_block_no_remainder, map_scatter=_xcd_block_no_remainder), want)
    assert not _same(m.run(map_count=_xcd_block_no_remainder), want)
    assert not _same(m.run(map_scatter=_xcd_block_no_remainder), want)
    # ... and only there: the same wrong map on grids of 8 and 16 blocks, and of 9 and 17
    rng = np.random.default_rng(8)
    for blocks in (8, 16, 9, 17):
        sizes = _residue_sizes(blocks)
        keys = _keys(rng, sum(sizes), MIXED, 8)
        vals = np.arange(sum(sizes), dtype=np.uint32)
        wrong = _PassModel(keys, vals, sizes, 0, 8).run(map_count=_xcd_block_no_remainder,
                                                        map_scatter=_xcd_block_no_remainder)
        assert _same(wrong, _expect(keys, vals, sizes, 8)) == (blocks % 8 == 0), blocks

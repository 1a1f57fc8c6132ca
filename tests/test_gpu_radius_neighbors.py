"""prg_radius_select_ragged_f64 / geometry.radius_neighbors_ragged / postprocess.radius_neighbors_hip on an MI355X.  Run with
`-m gpu`.

Everything is BIT-EXACT against `postprocess.radius_neighbors`: the matches of a row are `radius_pairs`', their order is (squared
distance in the shared float64 expression, then j), and tests/test_radius_neighbors_spec.py checks that definition against a
KD-tree on the CPU.  The kernel gives one wave to a query row, four rows to a workgroup, ranks 64 matches per pass and stages the
row's matches in LDS in chunks of 512: the query sizes below sit on both sides of 4, 64, 256 and 512, the limits on both sides of
a wave, and the rows with 700 and 1100 matches need several passes and several chunks."""
import numpy as np
import pytest
import torch

from pointreggpt_amd import postprocess as PP

pytestmark = pytest.mark.gpu

R = 0.5                    # ~8 matches per query row of a 1025-row cloud in the 64 m^3 box (tests/test_radius_pairs_spec.py)
ROW_SENTINEL, CORR_SENTINEL, TABLE_SENTINEL = -7, -77, -777
LEAD, SLACK = 2, 3         # table rows before the first pair's and after the last pair's that no query row owns
POISON = np.frombuffer(np.uint64(0x7FF8DEADBEEF0001).tobytes(), dtype=np.float64)[0]


@pytest.fixture(scope="module")
def L():
    from pointreggpt_amd import _lib
    _lib.load()
    return _lib


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cloud(rng, n):
    return rng.uniform([-2.0, -2.0, 0.0], [2.0, 2.0, 4.0], (n, 3))


def pack(segs, head=0, tail=0):
    """Ragged buffer with `head` / `tail` poisoned rows (NaN with a recognisable payload) outside every segment."""
    offs = np.zeros(len(segs) + 1, dtype=np.int64)
    offs[0] = head
    offs[1:] = head + np.cumsum([len(s) for s in segs])
    pts = np.concatenate([np.full((head, 3), POISON)] + [np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in segs]
                         + [np.full((tail, 3), POISON)], 0)
    return pts, offs


def launch(L, pairs, radius=R, limit=16, head=0, tail=0, index_base=None, pad=None):
    """count + fill + select on sentinel-filled outputs -> per-pair tables (host) and the per-row match counts from row_start.
    The table has LEAD rows in front and SLACK rows behind that belong to nobody; pts, row_start and corr must come back as they
    went in, and so must those rows."""
    lib = L.load()
    segs = [c for pair in pairs for c in pair]
    pts, offs = pack(segs, head, tail)
    total = len(pts)
    d_pts = D(pts if total else np.zeros((1, 3)))
    d_offs = D(offs)
    max_cloud = max(1, max(len(s) for s in segs))
    row_start = torch.full((max(total, 1) + 1,), ROW_SENTINEL, dtype=torch.int64, device="cuda")
    ws = torch.empty((int(lib.prg_radius_pairs_workspace_bytes(total)),), dtype=torch.uint8, device="cuda")
    rc = lib.prg_radius_count_ragged_f64(L.ptr(d_pts), L.ptr(d_offs), len(pairs), total, max_cloud, radius, L.ptr(row_start),
                                         L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc == 0, lib.prg_last_error()
    rs = row_start.cpu().numpy()
    K = int(rs[total])
    corr = torch.full((K + 8, 2), CORR_SENTINEL, dtype=torch.int32, device="cuda")    # slack rows: never read, never written
    rc = lib.prg_radius_fill_ragged_f64(L.ptr(d_pts), L.ptr(d_offs), len(pairs), max_cloud, radius, L.ptr(row_start), K, L.ptr(corr),
                                        L.stream_ptr())
    assert rc == 0, lib.prg_last_error()
    corr_before = corr.cpu().numpy()
    q_sizes = np.array([len(a) for a, _ in pairs], dtype=np.int64)
    t_offs = LEAD + np.concatenate([[0], np.cumsum(q_sizes)])
    Q = int(q_sizes.sum())
    table = torch.full((LEAD + Q + SLACK, limit), TABLE_SENTINEL, dtype=torch.int32, device="cuda")
    d_base = None if index_base is None else D(np.asarray(index_base, dtype=np.int32))
    d_pad = None if pad is None else D(np.asarray(pad, dtype=np.int32))
    rc = lib.prg_radius_select_ragged_f64(L.ptr(d_pts), L.ptr(d_offs), len(pairs), max_cloud, L.ptr(row_start),
                                          L.ptr(corr) if K else None, K, limit, L.ptr(D(t_offs)), L.ptr(d_base), L.ptr(d_pad),
                                          L.ptr(table), L.stream_ptr())
    assert rc == 0, lib.prg_last_error()
    torch.cuda.synchronize()
    if total:
        assert np.array_equal(bits(d_pts.cpu().numpy()), bits(pts))                   # pts unchanged, poison included
    assert np.array_equal(row_start.cpu().numpy(), rs)                                # select touches neither row_start
    assert np.array_equal(corr.cpu().numpy(), corr_before)                            # ... nor corr
    tab = table.cpu().numpy()
    assert np.all(tab[:LEAD] == TABLE_SENTINEL) and np.all(tab[LEAD + Q:] == TABLE_SENTINEL)   # nothing outside the query rows
    assert not np.any(tab[LEAD:LEAD + Q] == TABLE_SENTINEL)                           # every slot of every query row written
    got, counts = [], []
    for p in range(len(pairs)):
        got.append(tab[t_offs[p]:t_offs[p + 1]])
        counts.append(np.diff(rs[offs[2 * p]:offs[2 * p + 1] + 1]).astype(np.int32))
    return got, counts


def want_table(a, b, radius, limit, base=0, padv=None):
    idx, cnt = PP.radius_neighbors(a, b, radius, limit)
    padv = len(b) if padv is None else padv
    return np.where(idx < len(b), idx + np.int32(base), np.int32(padv)).astype(np.int32), cnt


def check(L, pairs, radius=R, limit=16, head=0, tail=0, index_base=None, pad=None):
    """Every pair's table and counts against the numpy specification, bit for bit; -> (tables, counts)."""
    got, counts = launch(L, pairs, radius, limit, head, tail, index_base, pad)
    for p, (a, b) in enumerate(pairs):
        want, cnt = want_table(a, b, radius, limit, 0 if index_base is None else index_base[p], None if pad is None else pad[p])
        assert got[p].shape == want.shape, (p, got[p].shape, want.shape)
        assert np.array_equal(got[p], want), (p, len(a), len(b), np.argwhere(got[p] != want)[:4].tolist())
        assert np.array_equal(counts[p], cnt)
    return got, counts


SIZES = [1, 3, 4, 5, 63, 64, 65, 257, 513, 1025]


@pytest.mark.parametrize("n", SIZES)
def test_query_sizes_against_the_spec(L, n):
    """n query rows against 1025 candidates (~8 matches per row), against 300 and against themselves — one launch."""
    rng = np.random.default_rng(n)
    a = cloud(rng, n)
    got, counts = check(L, [(cloud(rng, n), cloud(rng, 1025)), (cloud(rng, n), cloud(rng, 300)), (a, a)], limit=4)
    assert np.array_equal(got[2][:, 0], np.arange(n))                                 # a row's nearest row of itself is itself
    if n >= 63:
        assert (counts[0] > 4).any() and (counts[1] < 4).any()                        # truncated rows and padded rows


@pytest.mark.parametrize("limit", [1, 4, 16, 64, 65])
def test_limits_against_the_spec(L, limit):
    rng = np.random.default_rng(100 + limit)
    got, counts = check(L, [(cloud(rng, 1025), cloud(rng, 1025)), (cloud(rng, 513), cloud(rng, 300))], limit=limit)
    assert got[0].shape == (1025, limit)
    assert (counts[0] > 0).any() and (counts[1] == 0).any()


@pytest.mark.parametrize("nb,limit", [(700, 38), (700, 1024), (1100, 38), (1100, 1024)])
def test_rows_with_more_matches_than_a_wave_and_than_a_chunk(L, nb, limit):
    """Every candidate of a 0.3 m box is within 2 m of every query row: m = 700 is 11 passes of 64 targets over two chunks,
    m = 1100 three chunks; limit 1024 keeps every match of the 700 (and pads) and truncates the 1100."""
    rng = np.random.default_rng(nb + limit)
    b = rng.uniform(-0.15, 0.15, (nb, 3))
    a = rng.uniform(-0.15, 0.15, (9, 3))
    got, counts = check(L, [(a, b), (b[:5], b)], radius=2.0, limit=limit)
    assert np.all(counts[0] == nb) and np.all(counts[1] == nb)
    assert np.array_equal(got[1][:, 0], np.arange(5))
    if limit > nb:
        assert np.all(got[0][:, nb:] == nb) and np.all(np.sort(got[0][:, :nb], axis=1) == np.arange(nb))


def test_duplicates_that_straddle_chunk_and_wave_boundaries(L):
    """Equal distances are ordered by j: copies of one point at j = 63 / 64 (two passes), 511 / 512 (two chunks), 100 / 600 and
    three copies at 254 / 258 / 699."""
    rng = np.random.default_rng(31)
    b = rng.uniform(-0.15, 0.15, (700, 3))
    for lo, hi in ((63, 64), (511, 512), (100, 600), (254, 258), (254, 699)):
        b[hi] = b[lo]
    a = np.concatenate([b[[63, 511, 100, 254]], rng.uniform(-0.15, 0.15, (7, 3))])
    got, _ = check(L, [(a, b)], radius=2.0, limit=700)
    assert got[0][0, :2].tolist() == [63, 64] and got[0][1, :2].tolist() == [511, 512]
    assert got[0][2, :2].tolist() == [100, 600] and got[0][3, :3].tolist() == [254, 258, 699]
    got, _ = check(L, [(a, b)], radius=2.0, limit=1)                                  # the lower j wins the only slot
    assert got[0][:4, 0].tolist() == [63, 511, 100, 254]
    # the bound is strict: a candidate at exactly the radius is out, one ulp further in it is in
    q, cand = np.zeros((1, 3)), np.array([[0.5, 0, 0], [0, np.nextafter(0.5, 0), 0], [0, 0, -0.5], [0, 0, 0.25]])
    got, counts = check(L, [(q, cand)], radius=0.5, limit=3)
    assert got[0].tolist() == [[3, 1, 4]] and counts[0].tolist() == [2]


def test_nan_rows(L):
    rng = np.random.default_rng(32)
    a, b = cloud(rng, 600), cloud(rng, 520)
    a[0, 0] = a[17, 1] = a[599, 2] = np.nan
    b[0] = np.nan
    b[255, 1] = b[256, 2] = b[519, 0] = np.nan
    got, counts = check(L, [(a, b), (cloud(rng, 9), np.full((4, 3), np.nan)), (np.full((4, 3), np.nan), cloud(rng, 300))], limit=8)
    assert np.all(got[0][[0, 17, 599]] == 520) and not np.isin(got[0], [0, 255, 256, 519]).any()
    assert np.all(got[1] == 4) and np.all(got[2] == 300)
    assert (counts[0] > 0).any()


def test_empty_clouds_among_full_ones(L):
    rng = np.random.default_rng(33)
    e = np.zeros((0, 3))
    got, counts = check(L, [(e, cloud(rng, 300)), (cloud(rng, 300), e), (e, e), (cloud(rng, 600), cloud(rng, 600))])
    assert got[0].shape == (0, 16) and got[2].shape == (0, 16)
    assert np.all(got[1] == 0) and got[1].shape == (300, 16)                          # no candidates: all pads, and the pad is 0
    assert (counts[3] > 0).any()
    check(L, [(cloud(rng, 70), e)])                                                   # an empty list: corr is null
    check(L, [(e, cloud(rng, 70))])
    check(L, [(e, e), (e, e)], tail=4)
    check(L, [(e, e)])                                                                # ... and no row at all


@pytest.mark.parametrize("head,tail", [(5, 0), (0, 9), (301, 1777)])
def test_rows_outside_every_segment_are_left_alone(L, head, tail):
    rng = np.random.default_rng(head + tail)
    got, counts = check(L, [(cloud(rng, 700), cloud(rng, 513)), (cloud(rng, 64), cloud(rng, 1))], head=head, tail=tail)
    assert (counts[0] > 0).any()


def test_index_base_and_pad(L):
    """Given: a match is index_base[p] + j and an empty slot pad[p]; null: j and the candidate cloud's length."""
    rng = np.random.default_rng(34)
    pairs = [(cloud(rng, 130), cloud(rng, 257)), (cloud(rng, 65), cloud(rng, 520)), (cloud(rng, 5), np.zeros((0, 3)))]
    plain, _ = check(L, pairs, limit=8)
    moved, _ = check(L, pairs, limit=8, index_base=[1000, 0, 7], pad=[9999, 9999, -1])
    assert np.array_equal(moved[0], np.where(plain[0] < 257, plain[0] + 1000, 9999))
    assert np.all(moved[2] == -1) and np.all(plain[2] == 0)
    check(L, pairs, limit=8, index_base=[1000, 0, 7])                                 # one of the two given
    check(L, pairs, limit=8, pad=[9999, 9999, -1])


@pytest.mark.parametrize("n_pairs", [1, 3, 64])
def test_a_pair_does_not_depend_on_its_neighbours(L, n_pairs):
    """One pair alone gives the table it gives as the first, middle and last of n_pairs pairs (checked against the spec too)."""
    rng = np.random.default_rng(35)
    mine = (cloud(rng, 600), cloud(rng, 333))
    (alone,), _ = check(L, [mine], limit=4)
    assert (alone < 333).any() and (alone == 333).any()
    sizes = rng.integers(0, 700, size=(n_pairs, 2))
    others = [(cloud(rng, int(n)), cloud(rng, int(m))) for n, m in sizes]
    for pos in sorted({0, n_pairs // 2, n_pairs - 1}):
        pairs = list(others)
        pairs[pos] = mine
        if pos == 0:
            got, _ = check(L, pairs, limit=4)                     # every pair of one of the launches against the spec
        else:
            got, _ = launch(L, pairs, limit=4)
        assert np.array_equal(got[pos], alone)


def voxel_like(rng, n):
    """A 2.5 cm grid surface patch and the same patch with a 1 cm jitter: what a finished pair looks like at loader radii."""
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n] * 0.025
    a = np.concatenate([g, 1.5 + 0.1 * np.sin(3 * g[:, :1])], 1) + rng.uniform(-0.004, 0.004, (n, 3))
    b = a + rng.normal(0, 0.01, (n, 3))
    return a, b[rng.permutation(n)]


@pytest.mark.parametrize("radius,limit", [(0.0625, 16), (0.125, 38)])
def test_voxel_grid_like_clouds_at_the_network_radii(L, radius, limit):
    """At (0.0625, 16) most rows of the patch are truncated; (0.125, 38) is the second level's radius on the first level's
    density.  The patch against itself as well: the neighbours table of a level."""
    rng = np.random.default_rng(25)
    (a, b), (c, d) = voxel_like(rng, 1500), voxel_like(rng, 700)
    got, counts = check(L, [(a, b), (c, d), (a, a)], radius=radius, limit=limit)
    assert (counts[0] > limit).sum() > 750 and (counts[2] > limit).sum() > 750        # more than half of the rows truncated
    assert np.array_equal(got[2][:, 0], np.arange(1500))


def test_python_layers(L):
    """geometry.radius_neighbors_ragged returns device tensors; postprocess.radius_neighbors_hip splits them per pair."""
    from pointreggpt_amd import geometry as G
    rng = np.random.default_rng(36)
    e = np.zeros((0, 3))
    pairs = [(cloud(rng, 700), cloud(rng, 530)), (e, cloud(rng, 10)), (cloud(rng, 513), cloud(rng, 2)), (cloud(rng, 300), cloud(rng, 300) + 50.0),
             (cloud(rng, 7), e)]
    got = PP.radius_neighbors_hip(pairs, R, 6)
    assert len(got) == len(pairs)
    for (a, b), (idx, cnt) in zip(pairs, got):
        want, wcnt = PP.radius_neighbors(a, b, R, 6)
        assert idx.dtype == np.int32 and cnt.dtype == np.int32 and idx.shape == (len(a), 6) and cnt.shape == (len(a),)
        assert np.array_equal(idx, want) and np.array_equal(cnt, wcnt)
    assert (got[0][1] > 6).any() and np.all(got[3][0] == 300) and np.all(got[4][0] == 0)
    assert PP.radius_neighbors_hip([], R, 6) == []
    ((idx, cnt),) = PP.radius_neighbors_hip([(e, e)], R, 6)
    assert idx.shape == (0, 6) and cnt.shape == (0,)
    (far,) = PP.radius_neighbors_hip([pairs[3]], R, 6)                                 # K = 0 with rows present: no fill at all
    assert np.all(far[0] == 300) and np.all(far[1] == 0)
    pts, offs = pack([c for p in pairs[:3] for c in p])
    base, pad = D(np.array([10, 20, 30], dtype=np.int32)), D(np.array([-1, -2, -3], dtype=np.int32))
    table, to, count = G.radius_neighbors_ragged(D(pts), D(offs), 3, 700, R, 6, base, pad)
    assert table.is_cuda and table.dtype == torch.int32 and to.is_cuda and to.dtype == torch.int64
    assert count.is_cuda and count.dtype == torch.int32
    assert table.shape == (1213, 6) and count.shape == (1213,) and to.cpu().tolist() == [0, 700, 700, 1213]
    w0, c0 = want_table(*pairs[0], R, 6, 10, -1)
    w2, c2 = want_table(*pairs[2], R, 6, 30, -3)
    assert np.array_equal(table.cpu().numpy(), np.concatenate([w0, w2])) and np.array_equal(count.cpu().numpy(), np.concatenate([c0, c2]))


def test_error_paths(L):
    from pointreggpt_amd import geometry as G
    rng = np.random.default_rng(37)
    pts, offs = pack([cloud(rng, 40), cloud(rng, 50)])
    with pytest.raises(L.PrgError):
        G.radius_neighbors_ragged(torch.zeros((4, 3), dtype=torch.float64), torch.zeros(3, dtype=torch.int64), 1, 4, R, 4)
    with pytest.raises(L.PrgError):
        G.radius_neighbors_ragged(D(pts), D(offs), 1, 50, float("nan"), 4)
    with pytest.raises(L.PrgError):
        G.radius_neighbors_ragged(D(pts), D(offs), 1, 50, -1.0, 4)
    for limit in (0, -1, 1025):
        with pytest.raises(L.PrgError):
            G.radius_neighbors_ragged(D(pts), D(offs), 1, 50, R, limit)
    with pytest.raises(ValueError):
        PP.radius_neighbors_hip([(cloud(rng, 4), cloud(rng, 4))], R, 0)
    with pytest.raises(ValueError):
        PP.radius_neighbors_hip([(cloud(rng, 4), cloud(rng, 4))], float("inf"), 4)

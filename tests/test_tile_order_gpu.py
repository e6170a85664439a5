"""k_orderTiles (sol-r_amd/csrc/solr_post.hip), the tile sort of the cost-ordered launch, against the plain model of
tests/tile_order_model.py, through solr_hip_probe_order_tiles: the statistics the host decides by, the snapshot, the
split prefix, the heavy eighth and the bands of a streamed frame, and the bin of every entry of the order.  Within one
bin the tiles take their places in LDS atomic order, so a bin is compared as a set: the key sequence along `order`
must be the model's and every tile must be there once (four times, as consecutive quadrant parts, if split)."""
import numpy as np
import pytest

import engine_probes as E
import tile_order_model as M

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5

# (n, tiles per row): the BATCH x 1024 loop's edges, one and many trips, 1080p and 4K frames, the ragged frames that
# tests/test_streamed_frames_gpu.py streams (203 x 131, 203 x 121, 517 x 283)
SHAPES = [(1, 1), (2, 1), (63, 1), (1023, 1), (1024, 1), (1025, 1), (8191, 1), (8192, 1), (8193, 1),
          (32400, 240), (129600, 480), (26 * 17, 26), (26 * 16, 26), (65 * 36, 65)]
COSTS = ["zero", "equal", "outlier", "top-eighth", "top-eighth-plus-one", "power-law", "near-2^32", "class-boundaries"]


def costs(kind, n, seed=7):
    rng = np.random.default_rng(seed + n)
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "equal":
        return np.full(n, 777, np.uint32)
    if kind == "outlier":                          # one tile 1000 times the rest
        c = np.full(n, 50, np.uint32)
        c[int(rng.integers(n))] = 50000
        return c
    if kind.startswith("top-eighth"):              # two levels; the top class holds n / 8 tiles, or one more
        c = np.full(n, 5000, np.uint32)            # class 31 under a maximum of 10 000
        top = n // 8 + (1 if kind.endswith("one") else 0)
        c[rng.permutation(n)[:top]] = 10000
        return c
    if kind == "power-law":
        return np.minimum(1 + 200.0 * rng.pareto(1.2, n), 4.0e9).astype(np.uint32)
    if kind == "near-2^32":                        # (float)max + 1.f rounds to 2^32; the sum needs its high word
        c = (0xFFFFFFFF - rng.integers(0, 1 << 28, n)).astype(np.uint32)
        c[rng.permutation(n)[: max(1, n // 3)]] = rng.integers(0, 1 << 32, max(1, n // 3), dtype=np.uint64)
        c[0] = 0xFFFFFFFF
        c[min(1, n - 1)] = 2 ** 31 - 1            # rounds up to 2^31: class 32, not 31
        return c
    if kind == "class-boundaries":                 # maximum 1023: toClass = 1 / 16, a class is sixteen costs
        k = rng.integers(0, 64, n)
        c = (16 * k + rng.integers(-1, 2, n)).clip(0, 1023).astype(np.uint32)
        c[0] = 1023
        return c
    raise KeyError(kind)


def order_tiles(solr, cost, flights, cuts):
    hip = solr.hip_lib()
    E.declare(hip)
    n = len(cost)
    cost = np.ascontiguousarray(cost, np.uint32)
    order = np.full(M.order_words(n), SENTINEL, np.uint32)
    snapshot = np.full(n, SENTINEL, np.uint32)
    stats = np.full(8, SENTINEL, np.uint32)
    bands, heavy_share, first = cuts if cuts else (0, 0, [])
    first_tile = np.zeros(M.STREAM_BANDS_MAX + 1, np.int32)
    first_tile[:len(first)] = first
    status = hip.solr_hip_probe_order_tiles(n, cost.ctypes.data, flights, bands, heavy_share, first_tile.ctypes.data,
                                            order.ctypes.data, snapshot.ctypes.data, stats.ctypes.data)
    assert status == 1, "solr_hip_probe_order_tiles failed"
    return order, snapshot, stats


def check(solr, cost, flights, cuts, what):
    """one run of the kernel against the model"""
    n = len(cost)
    model = M.Model(cost, flights, cuts)
    order, snapshot, stats = order_tiles(solr, cost, flights, cuts)
    assert stats[:4].tolist() == model.stats, what
    assert stats[6:].tolist() == [SENTINEL, SENTINEL], what
    if flights == 0:
        assert (order == SENTINEL).all() and (snapshot == SENTINEL).all() and stats[5] == SENTINEL, what
        return stats
    assert np.array_equal(snapshot, cost), what
    assert stats[5] == model.split, (what, int(stats[5]), model.split)
    assert not (order == SENTINEL).any(), (what, "entries the kernel left untouched", np.flatnonzero(order == SENTINEL)[:8])
    key, part, tile = M.entries_as_keys(model, order)
    # a permutation: every tile once, a split tile four times as parts 1 ... 4 next to each other in the split prefix
    s = model.split
    prefix = M.SPLIT_PARTS * s
    assert (part[:prefix] == np.tile(np.arange(1, M.SPLIT_PARTS + 1), s)).all(), what
    quads = tile[:prefix].reshape(s, M.SPLIT_PARTS) if s else np.zeros((0, M.SPLIT_PARTS), np.int64)
    assert (quads == quads[:, :1]).all(), what
    whole = tile[prefix:n + (M.SPLIT_PARTS - 1) * s]
    assert (part[prefix:n + (M.SPLIT_PARTS - 1) * s] == 0).all(), what
    seen = np.concatenate([quads[:, 0], whole])
    assert len(seen) == n and np.array_equal(np.sort(seen), np.arange(n)), (what, "not a permutation")
    # the padding, and the bin of every entry
    assert (order[n + (M.SPLIT_PARTS - 1) * s:] == M.ORDER_NOTHING).all(), what
    bad = np.flatnonzero(key != model.seq_key)
    assert bad.size == 0, (what, "first entries out of their bins", bad[:8].tolist(), key[bad[:8]].tolist(),
                           model.seq_key[bad[:8]].tolist())
    assert np.array_equal(part, model.seq_part), what
    return stats


@pytest.mark.parametrize("n,tiles_x", SHAPES, ids=["n%d" % s[0] for s in SHAPES])
@pytest.mark.parametrize("kind", COSTS)
def test_the_tile_sort_against_the_model(solr, n, tiles_x, kind):
    cost = costs(kind, n)
    tile_rows = n // tiles_x
    serial = None
    for flights in (0, 1, 2, 4):
        for bands in (0, 3, 5, 8):
            if bands and flights == 0 and bands != 5:
                continue                       # (statistics only: the cuts are not read)
            shares = (8, 1) if bands else (8,)
            for share in shares:
                cuts = M.band_cuts(tiles_x, M.band_rows(tile_rows, bands), share) if bands else None
                what = "%s n=%d flights=%d bands=%d heavyShare=%d" % (kind, n, flights, bands, share)
                stats = check(solr, cost, flights, cuts, what)
                # the serial counts every run of the kernel
                assert serial is None or stats[4] == (serial + 1) & 0xFFFFFFFF, what
                serial = int(stats[4])


def test_the_model_is_not_vacuous_on_these_inputs():
    """the shapes and costs above reach every branch the model has: a split prefix, one at the limit of 256 tiles, the
    heavy eighth taken and refused, costs whose sum has a high word"""
    seen = set()
    for n, tiles_x in SHAPES:
        for kind in COSTS:
            cost = costs(kind, n)
            m = M.Model(cost, 1)
            if m.split:
                seen.add("split")
            if m.stats[2]:
                seen.add("sum beyond 32 bits")
            for share in (8, 1):
                b = M.Model(cost, 1, M.band_cuts(tiles_x, M.band_rows(n // tiles_x, 5), share))
                seen.add("heavy" if b.nb_heavy else "no heavy")
            if kind == "top-eighth" and n >= 8:
                assert M.Model(cost, 1, M.band_cuts(tiles_x, M.band_rows(n // tiles_x, 5))).nb_heavy == n // 8
            if kind == "top-eighth-plus-one" and n >= 8:
                assert M.Model(cost, 1, M.band_cuts(tiles_x, M.band_rows(n // tiles_x, 5))).nb_heavy == 0
    assert seen == {"split", "sum beyond 32 bits", "heavy", "no heavy"}, seen

"""Known answers of the k_orderTiles model (tests/tile_order_model.py), worked by hand from the kernel's expressions
(sol-r_amd/csrc/solr_post.hip:179-409) and imageStreamingCuts (solr_image_ring.hip:86-112).  No GPU: these pin the
model that tests/test_tile_order_gpu.py holds the kernel to."""
import numpy as np

import tile_order_model as M

NOTHING = -1


def runs(model):
    """the model's order as (key, part, tiles) runs over the entries before the padding"""
    out = []
    for pos in range(len(model.seq_key)):
        if model.seq_key[pos] == NOTHING:
            break
        if not out or out[-1][0] != model.seq_key[pos] or (model.seq_part[pos] != 0) != (out[-1][1] != 0):
            out.append([int(model.seq_key[pos]), int(model.seq_part[pos]), 0])
        out[-1][2] += 1
    return [tuple(r) for r in out]


def bin_of(model, key):
    return set(np.flatnonzero(model.key == key).tolist())


def test_band_cuts_of_the_frames_the_tests_stream():
    assert M.image_streaming_cuts(15) is None                          # fewer than sixteen tile rows: not streamed
    assert M.image_streaming_cuts(16) == [0, 3, 6, 9, 12, 16]
    assert M.image_streaming_cuts(17) == [0, 3, 6, 10, 13, 17]          # 203 x 131: the last row 3 pixels tall
    assert M.image_streaming_cuts(17, with_ids=True) == [0, 5, 11, 17]
    assert M.image_streaming_cuts(135) == [0, 27, 54, 81, 108, 135]    # 1920 x 1080
    assert M.band_rows(16, 8) == [0, 2, 4, 6, 8, 10, 12, 14, 16]
    assert M.band_cuts(26, [0, 3, 6, 10, 13, 17]) == (5, 8, [0, 78, 156, 260, 338, 442])
    # a band that starts at or before tile t holds t from there on (bandOfTile)
    tiles = np.arange(442)
    band = M.band_of_tile(tiles, 5, [0, 78, 156, 260, 338, 442])
    assert band[0] == 0 and band[77] == 0 and band[78] == 1 and band[259] == 2 and band[260] == 3 and band[441] == 4


def test_classes_at_their_boundaries_and_where_to_class_rounds():
    # max 1023: toClass = 64 / 1024 = 1 / 16 exactly; a class is sixteen costs
    max_cost, to_class, cls = M.classes([15, 16, 17, 1007, 1008, 1023, 0])
    assert max_cost == 1023 and to_class == np.float32(0.0625)
    assert cls.tolist() == [0, 1, 1, 62, 63, 63, 0]
    # max 2^32 - 1: (float)max + 1.f = 2^32, toClass = 2^-26.  2^31 - 1 rounds to 2^31 in binary32: class 32, where
    # exact arithmetic (31.99999997) would say 31; 2^32 - 129 rounds down to 2^32 - 256 (class 63); 2^32 - 1 rounds to
    # 2^32, 64 x 2^-26... = 64.0, clamped to 63
    max_cost, to_class, cls = M.classes([0xFFFFFFFF, 2 ** 31 - 1, 2 ** 31 - 129, 0xFFFFFF7F, 2 ** 26 - 1])
    assert to_class == np.float32(2.0 ** -26)
    assert cls.tolist() == [63, 32, 31, 63, 1]


def test_uniform_costs():
    model = M.Model(np.full(20, 100, np.uint32), flights=1)
    assert model.stats == [100, 2000, 0, 20] and model.split == 0
    assert (model.cls == 63).all()                                     # 100 x 64 / 101 = 63.4
    # bins (63 << 4) | (i & 15), descending: 15, 14 ... 4 alone, then {3, 19}, {2, 18}, {1, 17}, {0, 16}
    expect = [(1008 + j, 0, 1) for j in range(15, 3, -1)] + [(1008 + j, 0, 2) for j in range(3, -1, -1)]
    assert runs(model) == expect
    assert bin_of(model, 1011) == {3, 19}
    assert (model.seq_key[20:] == NOTHING).all() and len(model.seq_key) == 20 + 768


def test_one_outlier_is_split_into_four_quadrant_waves():
    cost = np.ones(1000, np.uint32)
    cost[5] = 1000
    for flights in (1, 2, 4):
        model = M.Model(cost, flights=flights)
        # mean 1.999, critical 3.998 (flights x 1999 / 5120 is less), above = (unsigned)(3.998 x 64 / 1001) + 1 = 1: the
        # smallest class >= 1 whose suffix holds <= 256 tiles is 1, and it holds the outlier alone
        assert model.stats == [1000, 1999, 0, 1000] and model.split == 1
        assert model.seq_key[:4].tolist() == [(63 << 4) | 5] * 4 and model.seq_part[:4].tolist() == [1, 2, 3, 4]
        # then the other 999 tiles, class 0, by i & 15 from 15 down (62 tiles have i & 15 = 15)
        assert runs(model)[1] == (15, 0, 62)
        assert (model.seq_part[4:1003] == 0).all() and (model.seq_key[1003:] == NOTHING).all()
    # in band mode no tile is split: the outlier is the heavy eighth, alone, first
    model = M.Model(cost, flights=1, cuts=(5, 8, [0, 200, 400, 600, 800, 1000]))
    assert model.split == 0 and model.heavy_from == 1 and model.nb_heavy == 1
    assert model.seq_key[0] == M.HEAVY | 63 and bin_of(model, M.HEAVY | 63) == {5}


def test_the_heavy_eighth_exactly_at_n_over_8_and_one_more():
    rows = M.image_streaming_cuts(16)                                  # 4 x 16 tiles, five bands
    cuts = M.band_cuts(4, rows)
    assert cuts == (5, 8, [0, 12, 24, 36, 48, 64])
    cost = np.full(64, 100, np.uint32)                                 # class 6 (100 x 64 / 1001 = 6.39)
    cost[56:] = 1000                                                   # eight tiles, class 63: exactly 64 / 8
    model = M.Model(cost, flights=1, cuts=cuts)
    assert model.heavy_from == 7 and model.nb_heavy == 8 and model.split == 0
    expect = [(M.HEAVY | 63, 0, 8)]
    for band, first, last in ((0, 0, 12), (1, 12, 24), (2, 24, 36), (3, 36, 48), (4, 48, 56)):
        half = (last - first) // 2
        expect += [(((7 - band) << 7) | (6 << 1) | 1, 0, half), (((7 - band) << 7) | (6 << 1), 0, half)]
    assert runs(model) == expect
    assert bin_of(model, M.HEAVY | 63) == set(range(56, 64))
    assert bin_of(model, (7 << 7) | (6 << 1) | 1) == {1, 3, 5, 7, 9, 11}
    # nine tiles of class 63: more than 64 / 8, so no class is heavy and they wait for their band (the last)
    cost[55] = 1000
    model = M.Model(cost, flights=1, cuts=cuts)
    assert model.heavy_from == 64 and model.nb_heavy == 0
    assert runs(model)[-4:] == [((3 << 7) | (63 << 1) | 1, 0, 5), ((3 << 7) | (63 << 1), 0, 4),
                                ((3 << 7) | (6 << 1) | 1, 0, 3), ((3 << 7) | (6 << 1), 0, 4)]
    assert bin_of(model, (3 << 7) | (63 << 1) | 1) == {55, 57, 59, 61, 63}
    # heavyShare 1: every class but class 0 may be heavy - here both classes are, and the empty ones below down to 1
    model = M.Model(cost, flights=1, cuts=(5, 1, cuts[2]))
    assert model.heavy_from == 1 and model.nb_heavy == 64
    assert runs(model) == [(M.HEAVY | 63, 0, 9), (M.HEAVY | 6, 0, 55)]


def test_all_zero_costs():
    model = M.Model(np.zeros(40, np.uint32), flights=2)
    assert model.stats == [0, 0, 0, 40] and model.to_class == np.float32(64.0)
    assert (model.cls == 0).all() and model.split == 0                # above = 1; no tile in classes >= 1
    assert runs(model) == [(j, 0, 3 if j < 8 else 2) for j in range(15, -1, -1)]
    # band mode: class 0 is never heavy
    model = M.Model(np.zeros(40, np.uint32), flights=1, cuts=(3, 8, [0, 10, 20, 40]))
    assert model.nb_heavy == 0 and model.heavy_from == 1
    assert runs(model)[0] == ((7 << 7) | 1, 0, 5) and bin_of(model, (7 << 7) | 1) == {1, 3, 5, 7, 9}


def test_a_split_prefix_of_whole_classes_and_its_limit():
    tiles = np.arange(1000)
    cost = np.where(tiles % 5 == 0, 1000, 1).astype(np.uint32)       # 200 tiles at 1000, 800 at 1
    model = M.Model(cost, flights=1)
    # mean 200.8, critical 401.6, above = (unsigned)(401.6 x 64 / 1001) + 1 = 26; classes >= 26 hold the 200
    assert model.stats == [1000, 200800, 0, 1000] and model.split == 200
    assert (model.seq_part[:800] == np.tile([1, 2, 3, 4], 200)).all()
    assert set((model.seq_key[:800] >> 4).tolist()) == {63}
    assert (model.seq_part[800:1600] == 0).all() and set((model.seq_key[800:1600] >> 4).tolist()) == {0}
    assert (model.seq_key[1600:] == NOTHING).all()
    # 300 tiles in class 63: more than SPLIT_TILES_MAX, and classes are split whole - none is
    cost = np.where(tiles % 10 < 3, 1000, 1).astype(np.uint32)
    model = M.Model(cost, flights=1)
    assert model.split == 0 and (model.seq_part[:1000] == 0).all()
    # two frames in flight raise the bar: flights x sum / 5120 = 2 x 300700 / 5120 = 117.5 < 2 x mean = 601.4 - the same
    assert M.Model(cost, flights=2).split == 0


def test_statistics_only_and_a_sum_beyond_32_bits():
    cost = np.full(3, 0xFFFFFFFF, np.uint32)
    model = M.Model(cost, flights=0)
    total = 3 * 0xFFFFFFFF
    assert model.stats == [0xFFFFFFFF, total & 0xFFFFFFFF, 2, 3]
    assert model.split is None and model.seq_key is None


def test_entries_map_back_to_keys():
    cost = np.array([5, 1, 9, 9], np.uint32)
    model = M.Model(cost, flights=1)
    order = np.full(M.order_words(4), M.ORDER_NOTHING, np.uint32)
    order[:4] = [2 | (1 << 26), 3, 0, 1]
    key, part, tile = M.entries_as_keys(model, order)
    assert tile[:4].tolist() == [2, 3, 0, 1] and part[:5].tolist() == [1, 0, 0, 0, -1]
    assert key[0] == model.key[2] and key[4] == NOTHING

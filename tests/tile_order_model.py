"""A plain model of k_orderTiles (sol-r_amd/csrc/solr_post.hip), the tile sort of the cost-ordered launch, and of the
band cuts the host hands it for a streamed frame (imageStreamingCuts, sol-r_amd/csrc/solr_image_ring.hip).

The kernel is a counting sort in LDS: every tile falls into a bin, the bins are laid out in descending order, and the
tiles of one bin take their places in the order in which their LDS atomics land.  So the order is fully determined up
to the order inside one bin: this model predicts the bin key at every position of `order`, and which entries are
quadrant parts of split tiles.  The binary32 expressions are the kernel's, evaluated in numpy float32 in the same
order (the library is built with -ffp-contract=off and correctly rounded division)."""
import numpy as np

SPLIT_PARTS = 4            # renderer.h: (1 << (2 * SOLR_SPLIT_LOG2)) with SOLR_SPLIT_LOG2 = 1
SPLIT_TILES_MAX = 256      # renderer.h
ORDER_NOTHING = 0xFFFFFFFF
ORDER_TILE_MASK = 0x03FFFFFF
ORDER_PART_SHIFT = 26
STREAM_BANDS_MAX = 8       # renderer.h SOLR_STREAM_BANDS_MAX
HEAVY = 1 << 10            # model-only key prefix of the band mode's heavy tiles (above every bin of the kernel)

f32 = np.float32


def order_words(n):
    """entries of `order`: four per split tile, one per other tile, ORDER_NOTHING to the end (solr_post.hip:174-178)"""
    return n + (SPLIT_PARTS - 1) * SPLIT_TILES_MAX


def band_rows(tile_rows, wanted):
    """imageStreamingCuts' loop (solr_image_ring.hip:104-111): first tile row of each of `wanted` bands, and tile_rows"""
    rows, row = [], 0
    for b in range(wanted):
        rows.append(row)
        row = max(row + 1, tile_rows * (b + 1) // wanted)
    rows.append(tile_rows)
    return rows


def image_streaming_cuts(tile_rows, with_ids=False):
    """imageStreamingCuts (solr_image_ring.hip:86-112) with streaming on: None for a frame of fewer than sixteen tile
    rows, else the first tile row of every band and tile_rows (five bands; three with the primitive ids)"""
    if tile_rows < 2 * STREAM_BANDS_MAX:
        return None
    return band_rows(tile_rows, 3 if with_ids else 5)


def band_cuts(tiles_x, rows, heavy_share=8):
    """BandCuts as decideStreamCuts makes them (solr_launch.hip:407-412): (bands, heavyShare, firstTile[0 ... bands])"""
    return len(rows) - 1, heavy_share, [r * tiles_x for r in rows]


def classes(cost):
    """(maxCost, toClass, class of every tile): solr_post.hip:241 and :257"""
    cost = np.asarray(cost, np.uint32)
    max_cost = int(cost.max()) if cost.size else 0
    to_class = f32(64.0) / (f32(max_cost) + f32(1.0))
    product = cost.astype(np.float64).astype(np.float32) * to_class       # (float)c * toClass, binary32
    cls = np.minimum(63, product.astype(np.int64))                         # min(63u, (unsigned)...)
    return max_cost, to_class, cls


def band_of_tile(tiles, bands, first_tile):
    """bandOfTile (solr_post.hip:161-168): the bands b = 1 ... 7 below `bands` whose first tile is at or before the tile"""
    band = np.zeros(len(tiles), np.int64)
    for b in range(1, STREAM_BANDS_MAX):
        if b < bands:
            band += tiles >= first_tile[b]
    return band


class Model:
    """What k_orderTiles leaves for `cost` (n = len(cost)), `flights` (the kernel's `sort`: 0 = statistics only) and
    `cuts` = (bands, heavyShare, firstTile) or None (bands = 0).

    stats     hostStats[0 ... 3]: max, sum lo, sum hi, n (solr_post.hip:225-231)
    split     hostStats[5]: tiles rendered as quadrant waves (solr_post.hip:380-384); 0 in band mode; None: not written
    key       per tile, the bin it is counted in; in band mode a heavy tile's key is HEAVY | class (classFirst)
    seq_key   per entry of `order` (order_words(n)): the key of the tile there, -1 for ORDER_NOTHING
    seq_part  per entry: 0 a whole tile, 1 ... 4 a quadrant of a split tile, -1 for ORDER_NOTHING
    None for seq_key / seq_part when flights == 0 (the kernel returns before it touches order)"""

    def __init__(self, cost, flights, cuts=None):
        cost = np.asarray(cost, np.uint32)
        n = len(cost)
        self.n = n
        tiles = np.arange(n, dtype=np.int64)
        total = int(cost.astype(np.uint64).sum())
        max_cost, to_class, cls = classes(cost)
        self.max_cost, self.to_class, self.cls = max_cost, to_class, cls
        self.stats = [max_cost, total & 0xFFFFFFFF, total >> 32, n]
        self.split, self.heavy_from, self.nb_heavy = None, 64, 0
        self.key = self.seq_key = self.seq_part = None
        if not flights:
            return
        bands = cuts[0] if cuts else 0
        if bands > 0:
            self._bands(cost, tiles, cls, cuts)
        else:
            self._by_cost(tiles, cls, total, flights)

    def _by_cost(self, tiles, cls, total, flights):
        """solr_post.hip:257-259 (bins), :340-409 (split, scatter)"""
        n = self.n
        self.key = (cls << 4) | (tiles & 15)
        # the split criterion (solr_post.hip:370-376): the smallest class c >= above whose suffix holds <= 256 tiles
        mean = f32(float(total)) / f32(max(n, 1))
        critical = np.maximum(f32(2.0) * mean, f32(flights) * f32(float(total)) / f32(5120.0))
        above = min(63, int(f32(critical) * self.to_class)) + 1
        count = np.bincount(cls, minlength=64)
        suffix = np.cumsum(count[::-1])[::-1]          # tiles in classes >= c
        split_class = 64
        for c in range(above, 64):
            if suffix[c] <= SPLIT_TILES_MAX:
                split_class = c
                break
        self.split = int(suffix[split_class]) if split_class < 64 else 0
        keys = np.sort(self.key)[::-1]
        seq_key = np.full(order_words(n), -1, np.int64)
        seq_part = np.full(order_words(n), -1, np.int64)
        s = self.split
        seq_key[:SPLIT_PARTS * s] = np.repeat(keys[:s], SPLIT_PARTS)
        seq_part[:SPLIT_PARTS * s] = np.tile(np.arange(1, SPLIT_PARTS + 1), s)
        seq_key[SPLIT_PARTS * s:n + (SPLIT_PARTS - 1) * s] = keys[s:]
        seq_part[SPLIT_PARTS * s:n + (SPLIT_PARTS - 1) * s] = 0
        self.seq_key, self.seq_part = seq_key, seq_part

    def _bands(self, cost, tiles, cls, cuts):
        """solr_post.hip:257-258 (bins), :261-334 (the heavy classes, the bands)"""
        n = self.n
        bands, heavy_share, first_tile = cuts
        band = band_of_tile(tiles, bands, first_tile)
        count = np.bincount(cls, minlength=64)
        # whole classes from 63 down, while they fit in n / heavyShare; class 0 is never heavy (solr_post.hip:276-285)
        up_to, first = 0, 64
        limit = n // max(heavy_share, 1)
        for c in range(63, 0, -1):
            if up_to + count[c] > limit:
                break
            up_to += int(count[c])
            first = c
        self.heavy_from, self.nb_heavy = first, up_to
        heavy = cls >= first
        self.key = np.where(heavy, HEAVY | cls, ((7 - band) << 7) | (cls << 1) | (tiles & 1))
        self.split = 0
        seq_key = np.full(order_words(n), -1, np.int64)
        seq_key[:n] = np.sort(self.key)[::-1]
        seq_part = np.full(order_words(n), -1, np.int64)
        seq_part[:n] = 0
        self.seq_key, self.seq_part = seq_key, seq_part


def entries_as_keys(model, order):
    """the key and part of every entry of a kernel's `order` under the model's keys (-1, -1 for ORDER_NOTHING; a tile
    index outside 0 ... n - 1 raises)"""
    order = np.asarray(order, np.uint32).astype(np.int64)
    nothing = order == ORDER_NOTHING
    tile = np.where(nothing, 0, order & ORDER_TILE_MASK)
    part = np.where(nothing, -1, (order >> ORDER_PART_SHIFT) & 31)
    if (tile >= model.n).any():
        raise IndexError("tile index outside the frame: %s" % order[tile >= model.n][:8].tolist())
    key = np.where(nothing, -1, model.key[tile])
    return key, part, np.where(nothing, -1, tile)

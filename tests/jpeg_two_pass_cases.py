"""What the tests of the optimised Huffman tables of the JPEG writer share (tests/test_jpeg_two_pass.py on the CPU,
tests/test_jpeg_two_pass_gpu.py on the device), next to tests/jpeg_entropy_cases.py, whose synthetic blocks are used too.
Nothing here shares code with sol-r_amd/csrc/jpeg_entropy.h:

  census(blocks, luma_blocks)       the symbols of a list of blocks, counted from the text of ITU T.81 F.1.2 (DC: the category
                                    of the difference to the component's last DC; AC: a (run << 4) + size symbol per
                                    coefficient, a ZRL per sixteen zeros in front of one, an end of block unless position 63
                                    is taken), in the order of jpn::Census - DC luma 12, DC chroma 12, AC luma 256, AC chroma 256
  model_tables(counts, variant)     jpge's optimize_huffman_table (jpge.cpp:353-397) restated in Python with a two-queue
                                    Huffman construction in place of the in-place one; `variant` restates one statement wrongly
  parse(file), decode(file)         a reader of baseline files that takes its tables from the file's own DHT segments: the
                                    coefficient blocks back, in MCU and zigzag order
  limit_18_case()                   the 18-symbol histogram of the fixtures' "limit_18" realised as coefficient blocks
  rare_dense_case()                 a group of 64 dense blocks whose 63 coefficients each carry one of their table's rarest
                                    symbols, behind enough blocks of other symbols for those to hold 16-bit codes
"""
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ("ties_reversed", "dummy_left_in", "dummy_from_shortest", "no_limit", "repair_wrong_length",
            "values_not_reversed")
SLOTS = ("dc_luma", "ac_luma", "dc_chroma", "ac_chroma")          # the order of a file's DHT segments (jpge.cpp:486-495)
CENSUS_SLICES = {"dc_luma": slice(0, 12), "dc_chroma": slice(12, 24), "ac_luma": slice(24, 280), "ac_chroma": slice(280, 536)}

_FIXTURES = None


def fixtures():
    """(jpeg_encoder.npz, jpeg_two_pass.npz), loaded once"""
    global _FIXTURES
    if _FIXTURES is None:
        _FIXTURES = (np.load(os.path.join(HERE, "golden", "jpeg_encoder.npz")),
                     np.load(os.path.join(HERE, "golden", "jpeg_two_pass.npz")))
    return _FIXTURES


def file_names():
    return sorted(k[5:] for k in fixtures()[1].files if k.startswith("file/"))


def table_names():
    return sorted({k.split("/")[1] for k in fixtures()[1].files if k.startswith("table/")})


def table(name):
    z = fixtures()[1]
    return z["table/%s/counts" % name], z["table/%s/bits" % name], z["table/%s/values" % name]


def file_case(name):
    """width, height, sampling, quality, blocks, jpge's one-pass file, jpge's two-pass file"""
    one, two = fixtures()
    width, height, h, v, quality, _, _ = (int(x) for x in one["params/" + name])
    return width, height, (h, v), quality, one["blocks/" + name], one["file/" + name].tobytes(), two["file/" + name].tobytes()


# ---- the census, from the text of F.1.2 ---------------------------------------------------------------------------------
def census(blocks, luma_blocks):
    counts = np.zeros(536, np.uint32)
    per_mcu = luma_blocks + 2
    prediction = [0, 0, 0]
    for index, block in enumerate(np.asarray(blocks).reshape(-1, 64).tolist()):
        within = index % per_mcu
        component = 0 if within < luma_blocks else within - luma_blocks + 1
        chroma = int(component > 0)
        difference = block[0] - prediction[component]
        prediction[component] = block[0]
        counts[12 * chroma + abs(difference).bit_length()] += 1
        ac = 24 + 256 * chroma
        run = 0
        for value in block[1:]:
            if value == 0:
                run += 1
                continue
            while run > 15:
                counts[ac + 0xF0] += 1
                run -= 16
            counts[ac + (run << 4) + abs(value).bit_length()] += 1
            run = 0
        if run:
            counts[ac + 0x00] += 1
    return counts


# ---- the table builder, restated ------------------------------------------------------------------------------------------
def _depths(counts):
    """how many leaves of the Huffman tree of ascending `counts` lie at each depth: {depth: leaves}.  Two queues - the
    leaves in order, the internal nodes in the order they were made - and of two equal candidates the leaf is taken, which is
    the choice the in-place algorithm makes"""
    n = len(counts)
    if n == 1:
        return {1: 1}
    parent = {}
    internal = []                      # (count, id) in creation order; ids n, n + 1, ...
    leaf = node = 0
    for made in range(n - 1):
        pair = []
        for _ in range(2):
            if leaf < n and (node >= len(internal) or not internal[node][0] < counts[leaf]):
                pair.append((counts[leaf], leaf))
                leaf += 1
            else:
                pair.append(internal[node])
                node += 1
        internal.append((pair[0][0] + pair[1][0], n + made))
        parent[pair[0][1]] = parent[pair[1][1]] = n + made
    out = {}
    for i in range(n):
        depth, at = 0, i
        while at in parent:
            at = parent[at]
            depth += 1
        out[depth] = out.get(depth, 0) + 1
    return out


def model_tables(counts, variant=None):
    """(bits, values) of one table as jpge builds it; bits has 16 entries (more under "no_limit" when codes are longer)"""
    symbols = [(1, -1)] + [(int(c), i) for i, c in enumerate(counts) if c]      # the dummy first
    if variant == "ties_reversed":
        order = sorted(range(len(symbols)), key=lambda k: (symbols[k][0], -k))
    else:
        order = sorted(range(len(symbols)), key=lambda k: symbols[k][0])        # (stable)
    ordered = [symbols[k] for k in order]
    depths = _depths([c for c, _ in ordered])
    longest = max(max(depths), 16)
    num = [0] * (longest + 2)
    for depth, leaves in depths.items():
        num[depth] += leaves
    if variant != "no_limit" and len(ordered) > 1:
        for length in range(17, longest + 1):
            num[16] += num[length]
            num[length] = 0
        total = sum(num[length] << (16 - length) for length in range(1, 17))
        while total != 1 << 16:
            num[16] -= 1
            candidates = range(1, 16) if variant == "repair_wrong_length" else range(15, 0, -1)
            for length in candidates:
                if num[length]:
                    num[length] -= 1
                    num[length + 1] += 2
                    break
            total -= 1
    bits = num[1:17] if variant != "no_limit" else num[1:longest + 1]
    if variant != "dummy_left_in":
        occupied = [i for i, b in enumerate(bits) if b]
        bits[occupied[0] if variant == "dummy_from_shortest" else occupied[-1]] -= 1
    values = [s for _, s in ordered if s >= 0]
    if variant != "values_not_reversed":
        values = values[::-1]
    return bits, values


def model_huffman(counts536):
    """the four tables of a census, in DHT order: [(bits, values)]"""
    return [model_tables(counts536[CENSUS_SLICES[slot]]) for slot in SLOTS]


# ---- a reader with the file's own tables ----------------------------------------------------------------------------------
def parse(data):
    """{"width", "height", "sampling", "tables": {(class, id): (bits, values)}, "dht_order", "header_bytes", "scan"}"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    out = {"tables": {}, "dht_order": []}
    at = 2
    while True:
        assert data[at] == 0xFF
        marker = data[at + 1]
        length = struct.unpack(">H", data[at + 2:at + 4])[0]
        body = data[at + 4:at + 2 + length]
        if marker == 0xC0:
            _, out["height"], out["width"], components = struct.unpack(">BHHB", body[:6])
            assert components == 3
            out["sampling"] = (body[7] >> 4, body[7] & 15)
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                key = (body[k] >> 4, body[k] & 15)
                bits = list(body[k + 1:k + 17])
                out["tables"][key] = (bits, list(body[k + 17:k + 17 + sum(bits)]))
                out["dht_order"].append(key)
                k += 17 + sum(bits)
        at += 2 + length
        if marker == 0xDA:
            break
    out["header_bytes"] = at
    out["scan"] = data[at:-2]
    return out


def _decoder(bits, values):
    """annex C: {(length, code): symbol}"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = values[k]
            code, k = code + 1, k + 1
        code <<= 1
    return out


def decode(data):
    """the coefficient blocks of a baseline file, (n, 64) int16 in MCU and zigzag order, by the file's own tables (F.2.2)"""
    p = parse(data)
    h, v = p["sampling"]
    luma_blocks = h * v
    nb_blocks = -(-p["width"] // (8 * h)) * -(-p["height"] // (8 * v)) * (luma_blocks + 2)
    scan = p["scan"].replace(b"\xff\x00", b"\xff")
    stream = bin(int.from_bytes(b"\x01" + scan, "big"))[3:]
    decoders = {key: _decoder(*t) for key, t in p["tables"].items()}
    at = 0

    def symbol(table):
        nonlocal at
        code = 0
        for length in range(1, 17):
            code = (code << 1) | int(stream[at + length - 1])
            if (length, code) in table:
                at += length
                return table[(length, code)]
        raise AssertionError("no code at bit %d" % at)

    def amplitude(size):
        nonlocal at
        if size == 0:
            return 0
        raw = int(stream[at:at + size], 2)
        at += size
        return raw if raw >> (size - 1) else raw - (1 << size) + 1

    blocks = np.zeros((nb_blocks, 64), np.int16)
    prediction = [0, 0, 0]
    for index in range(nb_blocks):
        within = index % (luma_blocks + 2)
        component = 0 if within < luma_blocks else within - luma_blocks + 1
        chroma = int(component > 0)
        prediction[component] += amplitude(symbol(decoders[(0, chroma)]))
        blocks[index, 0] = prediction[component]
        k = 1
        while k < 64:
            s = symbol(decoders[(1, chroma)])
            if s == 0x00:
                break
            if s == 0xF0:
                k += 16
                continue
            k += s >> 4
            blocks[index, k] = amplitude(s & 15)
            k += 1
    tail = stream[at:]
    assert len(tail) < 8 and set(tail) <= {"1"}, "what follows the last block is not a byte's completion with one-bits"
    return blocks


# ---- blocks made for the tables ---------------------------------------------------------------------------------------------
def _case(name, sampling, mcus_per_row, mcu_rows, blocks):
    blocks = np.ascontiguousarray(blocks, np.int16).reshape(-1, 64)
    assert len(blocks) == mcus_per_row * mcu_rows * (sampling[0] * sampling[1] + 2), name
    return {"name": name, "sampling": sampling, "quality": 85, "width": mcus_per_row * 8 * sampling[0],
            "height": mcu_rows * 8 * sampling[1], "blocks": blocks}


def limit_18_case():
    """Luma blocks whose AC symbols are exactly the fixtures' "limit_18" histogram - 1, 2, 3, 5, 8 ... over the end of block,
    (run 1, size 1 ... 8) and (run 0, size 1 ... 9), 10 944 symbols - so that the luma AC table is that fixture's and the
    16-bit limit engages in a file.  Every block but the last is filled to position 63 (no end of block), the last ends
    early: the one end of block the histogram has.  Chroma blocks are zero.  2x2: 4 luma blocks per MCU."""
    counts, _, _ = table("limit_18")
    assert int(counts[0x00]) == 1
    # the symbols of two positions first, the frequent ones of a single position behind them and wherever one position is left
    tokens = [s for s in range(1, 256) if s >> 4 for _ in range(int(counts[s]))]
    singles = [s for s in range(1, 256) if not s >> 4 for _ in range(int(counts[s]))]
    assert len(tokens) + len(singles) + 1 == int(counts.sum()) and all(s >> 4 == 1 for s in tokens)
    luma = []
    while tokens or singles:
        block, at = np.zeros(64, np.int16), 1
        while at < 64 and (tokens or singles):
            s = tokens.pop() if tokens and at < 63 else singles.pop() if singles else None
            if s is None:
                break
            at += s >> 4
            block[at] = (1 << ((s & 15) - 1)) * (-1 if at % 2 else 1)
            at += 1
        luma.append(block)
    assert len(luma) % 4 == 0 and luma[-1][63] == 0 and all(b[63] != 0 for b in luma[:-1])
    mcus = len(luma) // 4
    blocks = np.zeros((mcus, 6, 64), np.int16)
    blocks[:, :4] = np.array(luma).reshape(mcus, 4, 64)
    return _case("limit_18_blocks", (2, 2), mcus, 1, blocks)


def rare_dense_case(chain=8):
    """A group of 64 dense blocks - all 63 coefficients non-zero - each coefficient carrying one of the ten (run 0, size s)
    symbols, which are the rarest of their table and hold its longest codes: in front of the group come blocks of
    (run 1, size s) symbols with counts that grow like 1, 2, 3, 5, 8 ... from the group's own, `chain` of them.  1x1
    sampling, an MCU's three blocks alike in front: both AC tables have the shape.  The group's first block is a multiple of
    64: it is one workgroup's, and its piece of the stream is the longest of the case.

    (That all of a dense group's symbols hold 16-bit codes - the piece of 64 x 1665 bits - takes a table in which a symbol
    met 22 x 63 / 10 = 139 times has a probability near 2^-15: some 4 million symbols per table, 200 000 blocks.  The
    16-bit codes themselves are in limit_18_case; here the longest pieces are.)"""
    rare = np.zeros((64, 64), np.int16)
    for b in range(64):
        sizes = (np.arange(63) + b) % 10 + 1
        rare[b, 1:] = ((1 << sizes) - 1) * np.where((np.arange(63) + b) % 2, -1, 1)
    rare[:, 0] = np.where(np.arange(64) % 2, 1000, -1000)            # (DC differences of category 11)
    fib = [1, 2]
    while len(fib) < chain:
        fib.append(fib[-1] + fib[-2])
    front = []
    for size, multiple in zip(range(1, 11), fib):
        block = np.zeros(64, np.int16)
        block[2::2] = 1 << (size - 1)                                 # 31 symbols (run 1, size) and an end of block
        front += [block] * (-(-22 * 63 * multiple // 31))
    front = np.array(front, np.int16)
    nb_front = -(-len(front) * 3 // 192) * 192                       # whole MCUs, and the group starts a workgroup
    mcus = (nb_front + 66) // 3                                      # (+ 2 blocks: 64 is no multiple of 3)
    side = int(np.ceil(np.sqrt(mcus)))
    rows = -(-mcus // side)
    blocks = np.zeros((side * rows * 3, 64), np.int16)
    blocks[:len(front) * 3].reshape(-1, 3, 64)[:] = front[:, None, :]
    blocks[nb_front:nb_front + 64] = rare
    case = _case("rare_dense_group", (1, 1), side, rows, blocks)
    case["group"] = nb_front
    return case

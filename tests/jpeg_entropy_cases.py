"""Synthetic coefficient blocks that steer the entropy stage of the JPEG writer (sol-r_amd/csrc/jpeg_entropy.h) to its
edges - not pictures: every case is a list of quantised blocks in MCU and zigzag order made for one property of the bit
stream, by a generator that is a function of a committed seed (SEEDS; tests/jpeg_entropy_cases.py --search finds them on
the CPU) and that counts the edges its blocks reach.  edges(case) does the counting on a text model of the coder kept here
(model_scan: one pass, a bit at a time, nothing shared with the header), and cases() asserts that every count a case is
there for is greater than zero.

What the issue's list becomes:
  eob_only_444 / _422 / _420   blocks of only DC 0 (an end-of-block and nothing else) in the three samplings
  last_position                a coefficient at position 63: no end-of-block
  zero_runs                    runs of 15, 16, 17, 31, 32, 47 and 62 zeros in front of a coefficient (0, 1, 1, 1, 2, 2, 3 ZRL)
  dc_categories                every DC category 0 ... 11 with both signs, in luma and in chroma
  ac_categories                every AC category 1 ... 10 with both signs, at both ends of each category
  densest_sparsest             the longest block the tables allow next to the shortest.  (The header's bound is 22 + 63 * 26 =
                               1660 bits; the 22 is the chroma DC's and the 26 the luma AC's, so no single block reaches it:
                               the longest real one is a luma block of 20 + 63 * 26 = 1658 bits, and that is the one here)
  dc_predecessors              2x2 MCUs in two MCU rows with a different DC in every block: differences inside an MCU's luma
                               blocks, across MCUs and across the end of an MCU row
  ff_across_blocks             0xFF bytes of the unstuffed stream whose bits belong to two blocks
  ff_run                       three 0xFF in a row.  Four cannot happen inside the domain: a code word is never all ones, the
                               longest run of one-bits is an 11-bit DC amplitude followed by the 15 ones of a 16-bit code, 26
                               bits, and four bytes take 32
  ff_chunk_edge                0xFF as the last byte of a stuffing chunk and as the first byte of the next
  ends_on_byte, ends_with_1 ... ends_with_7    the stream's length modulo 8
  last_byte_ff                 the completed last byte comes out as 0xFF (and is stuffed)
  blocks_63, _64, _66, _126, _128, _129    block counts around the blocks per workgroup c = 64 and 2c.  A count is a
                               multiple of 3, 4 or 6 blocks per MCU: 65 (c + 1) is none, 66 stands in, and 129 is 2c + 1
  bytes_255, _256, _257, _511, _512, _513      unstuffed stream lengths around the bytes per stuffing chunk and twice that
  one_mcu                      one MCU alone
  row_of_512_mcus              512 MCUs in one row
(The two prefix sums on the device are hipcub's, whose tile is not a constant of the header: nothing to put counts around.)
Under 40 cases, none above 4096 blocks."""
import sys

import numpy as np

# ---- ITU T.81 annex K.3, typed in from the standard's tables K.3 - K.6 as (code lengths, symbols) ------------------------
_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))


def _ac_symbols(order):
    return [int(order[i:i + 2], 16) for i in range(0, len(order), 2)]


_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], _ac_symbols(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], _ac_symbols(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def _codes(bits, values):
    """annex C: symbol -> (code, length)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[values[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


TABLES = ((_codes(*_DC_LUMA), _codes(*_AC_LUMA)), (_codes(*_DC_CHROMA), _codes(*_AC_CHROMA)))
VARIANTS = ("eob_always", "zrl_at_15", "negative_without_minus_one", "tail_zeros", "tail_byte_not_stuffed",
            "stuffing_counted_per_word", "dc_from_any_component", "offsets_in_32_bits")


def _amplitude(value, size, variant):
    if value < 0 and variant != "negative_without_minus_one":
        value -= 1
    return value & ((1 << size) - 1)


def model_scan(blocks, sampling, variant=None):
    """The entropy-coded segment of `blocks` by the text of ITU T.81 F.1.2 and B.1.1.5 and jpge's closing seven one-bits,
    one pass; `variant` restates one statement wrongly.  Returns (bytes, the bit offset of every block and of the end, the
    unstuffed bytes with the last one completed)."""
    luma_blocks = sampling[0] * sampling[1]
    per_mcu = luma_blocks + 2
    bits, offsets, total = [], [], 0
    prediction = [0, 0, 0]
    last = 0
    for index, block in enumerate(np.asarray(blocks).tolist()):
        offsets.append(total)
        within = index % per_mcu
        c = 0 if within < luma_blocks else within - luma_blocks + 1
        dc, ac = TABLES[c > 0]
        difference = block[0] - (last if variant == "dc_from_any_component" else prediction[c])
        prediction[c] = last = block[0]
        size = abs(difference).bit_length()
        out = [dc[size]]
        if size:
            out.append((_amplitude(difference, size, variant), size))
        run = 0
        for value in block[1:]:
            if value == 0:
                run += 1
                continue
            while run >= (15 if variant == "zrl_at_15" else 16):
                out.append(ac[0xF0])
                run -= 16 if variant != "zrl_at_15" else 15
            size = abs(value).bit_length()
            out.append(ac[(run << 4) | size])
            out.append((_amplitude(value, size, variant), size))
            run = 0
        if run or variant == "eob_always":
            out.append(ac[0x00])
        for value, length in out:
            bits.append(format(value, "0%db" % length))
            total += length
    offsets.append(total)
    if variant == "offsets_in_32_bits":
        offsets = [o & 0xFFFFFFFF for o in offsets]
    stream = "".join(bits)
    stream += ("0" if variant == "tail_zeros" else "1") * (-len(stream) % 8)
    unstuffed = bytes(int(stream[i:i + 8], 2) for i in range(0, len(stream), 8))
    scan = bytearray()
    if variant == "stuffing_counted_per_word":
        for i in range(0, len(unstuffed), 4):
            word = unstuffed[i:i + 4]
            at = word.find(b"\xff")
            scan += word if at < 0 else word[:at + 1] + b"\x00" + word[at + 1:]
    else:
        for i, byte in enumerate(unstuffed):
            scan.append(byte)
            if byte == 0xFF and not (variant == "tail_byte_not_stuffed" and i == len(unstuffed) - 1):
                scan.append(0)
    return bytes(scan), offsets, unstuffed


def edges(case):
    """what the case's stream reaches, counted on the model"""
    blocks, sampling = case["blocks"], case["sampling"]
    luma_blocks = sampling[0] * sampling[1]
    per_mcu = luma_blocks + 2
    _, offsets, unstuffed = model_scan(blocks, sampling)
    total = offsets[-1]
    n = {"blocks": len(blocks), "bits": total, "unstuffed_bytes": len(unstuffed)}
    n["eob_only"] = int((np.abs(blocks).sum(axis=1) == 0).sum())
    n["no_eob"] = int((blocks[:, 63] != 0).sum())
    for run in (15, 16, 17, 31, 32, 47, 62):
        n["run_%d" % run] = 0
    n["dc_pos"], n["dc_neg"], n["ac_pos"], n["ac_neg"] = set(), set(), set(), set()
    n["dc_across_row"] = n["dc_inside_mcu"] = 0
    prediction = [0, 0, 0]
    mcus_per_row = case["mcus_per_row"]
    for index, block in enumerate(blocks.tolist()):
        within, mcu = index % per_mcu, index // per_mcu
        c = 0 if within < luma_blocks else within - luma_blocks + 1
        d = block[0] - prediction[c]
        if d and 0 < within < luma_blocks:
            n["dc_inside_mcu"] += 1
        if d and mcu and mcu % mcus_per_row == 0 and (within == 0 or within >= luma_blocks):
            n["dc_across_row"] += 1
        prediction[c] = block[0]
        (n["dc_neg"] if d < 0 else n["dc_pos"]).add((c > 0, abs(d).bit_length()))
        run = 0
        for value in block[1:]:
            if value == 0:
                run += 1
                continue
            if "run_%d" % run in n:
                n["run_%d" % run] += 1
            (n["ac_neg"] if value < 0 else n["ac_pos"]).add(abs(value).bit_length())
            run = 0
    n["longest_block"] = max(b - a for a, b in zip(offsets, offsets[1:]))
    n["shortest_block"] = min(b - a for a, b in zip(offsets, offsets[1:]))
    inner = set(o // 8 for o in offsets[1:-1] if o % 8)  # bytes that hold the end of one block and the start of the next
    ff = [i for i, byte in enumerate(unstuffed) if byte == 0xFF]
    n["ff"] = len(ff)
    n["ff_across_blocks"] = sum(1 for i in ff if i in inner)
    longest = current = 0
    for i, byte in enumerate(unstuffed):
        current = current + 1 if byte == 0xFF else 0
        longest = max(longest, current)
    n["ff_longest_run"] = longest
    n["ff_last_of_chunk"] = sum(1 for i in ff if i % 256 == 255)
    n["ff_first_of_chunk"] = sum(1 for i in ff if i % 256 == 0 and i)
    n["ff_both_sides_of_a_chunk_edge"] = sum(1 for i in ff if i % 256 == 255 and i + 1 < len(unstuffed) and
                                             unstuffed[i + 1] == 0xFF)
    n["tail_bits"] = -total % 8
    n["last_byte_ff"] = int(unstuffed[-1] == 0xFF)
    return n


# ---- the generators -------------------------------------------------------------------------------------------------------
def _case(name, sampling, mcus_per_row, mcu_rows, blocks, wanted):
    blocks = np.ascontiguousarray(blocks, dtype=np.int16).reshape(-1, 64)
    per_mcu = sampling[0] * sampling[1] + 2
    assert len(blocks) == mcus_per_row * mcu_rows * per_mcu and len(blocks) <= 4096, name
    return {"name": name, "sampling": sampling, "mcus_per_row": mcus_per_row, "mcu_rows": mcu_rows, "quality": 85,
            "width": mcus_per_row * 8 * sampling[0], "height": mcu_rows * 8 * sampling[1], "blocks": blocks,
            "wanted": wanted}


def _random_blocks(rng, n, density, ones=0.5, top=10):
    """n blocks; a coefficient is non-zero with probability `density`, its category uniform in 1 ... top, and with
    probability `ones` it is the largest value of its category (an amplitude of all ones)"""
    size = rng.randint(1, top + 1, (n, 64))
    largest = (1 << size) - 1
    value = np.where(rng.rand(n, 64) < ones, largest, rng.randint(0, 1 << 30, (n, 64)) % (largest - (largest >> 1)) +
                     (largest >> 1) + 1)
    value = np.where(rng.rand(n, 64) < 0.5, value, -value) * (rng.rand(n, 64) < density)
    value[:, 0] = rng.randint(-1000, 1001, n)  # (differences of two stay within +-2000: category 11 at most)
    return value.astype(np.int16)


def _dense(seed, n_mcus, sampling=(1, 1), density=0.9, ones=0.7):
    rng = np.random.RandomState(seed)
    return _random_blocks(rng, n_mcus * (sampling[0] * sampling[1] + 2), density, ones)


def _sparse(seed, n_mcus, sampling=(1, 1), density=0.03):
    rng = np.random.RandomState(seed)
    return _random_blocks(rng, n_mcus * (sampling[0] * sampling[1] + 2), density, 0.3, top=6)


SEEDS = {}
SEARCHES = {}  # name -> (make(seed) -> case, accept(edges) -> bool)


def _searched(name, make, accept):
    SEARCHES[name] = (make, accept)


def _zero_runs():
    runs = (15, 16, 17, 31, 32, 47, 62)
    blocks = np.zeros((63, 64), np.int16)
    for i in range(63):
        blocks[i, 1 + runs[i % 7]] = (-1) ** i * (1 + i % 5)
        if runs[i % 7] < 40 and i % 2:
            blocks[i, 63] = 3  # (a second run behind the first)
    return blocks


def _dc_categories():
    """per component: 0, then for every category its smallest and its largest difference, up and down again"""
    steps = [0]
    for c in range(1, 12):
        for d in (1 << (c - 1), (1 << c) - 1):
            steps += [d, -d]
    chain = np.cumsum(steps)
    blocks = np.zeros((len(chain) * 3, 64), np.int16)
    for c in range(3):
        blocks[c::3, 0] = chain
    return blocks


def _ac_categories():
    values = []
    for c in range(1, 11):
        for v in (1 << (c - 1), (1 << c) - 1):
            values += [v, -v]
    blocks = np.zeros((12, 64), np.int16)
    for b in range(12):
        for i, v in enumerate(values):
            blocks[b, 1 + (i * (b % 4 + 1) + b) % 63] = v
    return blocks


def _densest_sparsest():
    blocks = np.zeros((9, 64), np.int16)
    blocks[3, 0] = 2047
    blocks[3, 1:] = np.where(np.arange(63) % 2, -1023, 1023)
    return blocks  # (the next luma block comes down again: a difference of -2047, category 11)


def _dc_predecessors():
    rng = np.random.RandomState(7)
    blocks = np.zeros((2 * 3 * 6, 64), np.int16)
    blocks[:, 0] = rng.permutation(np.arange(-900, 900, 50))[:36]
    blocks[:, 5] = 1
    return blocks


def _fixed():
    zero = lambda n: np.zeros((n, 64), np.int16)
    last = _sparse(11, 8, density=0.05)
    last[::2, 63] = np.where(np.arange(len(last[::2])) % 2, -5, 9)
    return [
        _case("eob_only_444", (1, 1), 5, 1, zero(15), ["eob_only"]),
        _case("eob_only_422", (2, 1), 5, 1, zero(20), ["eob_only"]),
        _case("eob_only_420", (2, 2), 3, 2, zero(36), ["eob_only"]),
        _case("last_position", (1, 1), 8, 1, last, ["no_eob"]),
        _case("zero_runs", (1, 1), 7, 3, _zero_runs(), ["run_%d" % r for r in (15, 16, 17, 31, 32, 47, 62)]),
        _case("dc_categories", (1, 1), len(_dc_categories()) // 3, 1, _dc_categories(), ["dc_all"]),
        _case("ac_categories", (2, 1), 3, 1, _ac_categories(), ["ac_all"]),
        _case("densest_sparsest", (1, 1), 3, 1, _densest_sparsest(), ["densest", "sparsest"]),
        _case("dc_predecessors", (2, 2), 3, 2, _dc_predecessors(), ["dc_across_row", "dc_inside_mcu"]),
        _case("one_mcu", (2, 2), 1, 1, _dense(5, 1, (2, 2), 0.4), ["one_mcu"]),
        _case("row_of_512_mcus", (1, 1), 512, 1, _dense(6, 512, (1, 1), 0.15, 0.5), ["row_512"]),
    ]


_searched("ff_across_blocks", lambda s: _case("ff_across_blocks", (1, 1), 20, 1, _dense(s, 20), ["ff_across_blocks"]),
          lambda n: n["ff_across_blocks"] >= 3)
def _ff_run(seed):
    """the longest run of one-bits there is - a DC difference of +2047 (11 ones), then run 15 / category 10 (the code with 15
    ones) - in every other luma block, between sparse blocks that shift it to every alignment"""
    blocks = _sparse(seed, 16, density=0.1)
    blocks[0::3] = 0
    blocks[0::6, 0] = 2047
    blocks[0::6, 16] = 1023
    return _case("ff_run", (1, 1), 16, 1, blocks, ["ff_run"])


_searched("ff_run", _ff_run, lambda n: n["ff_longest_run"] >= 3)
_searched("ff_chunk_edge", lambda s: _case("ff_chunk_edge", (2, 1), 40, 2, _dense(s, 80, (2, 1), ones=0.9),
                                           ["ff_chunk_edge"]),
          lambda n: n["ff_both_sides_of_a_chunk_edge"] >= 1)
_searched("ends_on_byte", lambda s: _case("ends_on_byte", (1, 1), 2, 1, _sparse(s, 2, density=0.2), ["tail_0"]),
          lambda n: n["tail_bits"] == 0)
for _k in range(1, 8):
    _searched("ends_with_%d" % _k, (lambda k: lambda s: _case("ends_with_%d" % k, (1, 1), 2, 1, _sparse(s, 2, density=0.2),
                                                               ["tail_%d" % k]))(_k),
              (lambda k: lambda n: (8 - n["tail_bits"]) % 8 == k)(_k))
_searched("last_byte_ff", lambda s: _case("last_byte_ff", (1, 1), 1, 1, _dense(s, 1, ones=1.0), ["last_byte_ff"]),
          lambda n: n["last_byte_ff"] == 1 and n["tail_bits"] > 0)
for _count, _sampling in ((63, (1, 1)), (64, (2, 1)), (66, (2, 2)), (126, (2, 2)), (128, (2, 1)), (129, (1, 1))):
    _per = _sampling[0] * _sampling[1] + 2
    SEARCHES["blocks_%d" % _count] = (
        (lambda count, sampling, per: lambda s: _case("blocks_%d" % count, sampling, count // per, 1,
                                                      _dense(s, count // per, sampling, 0.5), ["blocks_%d" % count]))(
            _count, _sampling, _per), lambda n: n["ff"] > 0)
for _bytes in (255, 256, 257, 511, 512, 513):
    SEARCHES["bytes_%d" % _bytes] = (
        (lambda nb: lambda s: _case("bytes_%d" % nb, (1, 1), nb // 24, 1, _sparse(s, nb // 24), ["bytes_%d" % nb]))(_bytes),
        (lambda nb: lambda n: n["unstuffed_bytes"] == nb)(_bytes))

SEEDS.update({
    "ff_across_blocks": 0,
    "ff_run": 0,
    "ff_chunk_edge": 1,
    "ends_on_byte": 10,
    "ends_with_1": 2,
    "ends_with_2": 0,
    "ends_with_3": 12,
    "ends_with_4": 15,
    "ends_with_5": 3,
    "ends_with_6": 4,
    "ends_with_7": 13,
    "last_byte_ff": 7,
    "blocks_63": 0,
    "blocks_64": 0,
    "blocks_66": 0,
    "blocks_126": 0,
    "blocks_128": 0,
    "blocks_129": 0,
    "bytes_255": 3,
    "bytes_256": 110,
    "bytes_257": 78,
    "bytes_511": 42,
    "bytes_512": 112,
    "bytes_513": 14,
})


def _met(case, n):
    """every edge the case is there for, as a count greater than zero"""
    counts = {}
    for wanted in case["wanted"]:
        if wanted == "dc_all":
            both = [(chroma, c) for chroma in (False, True) for c in range(1, 12)]
            counts[wanted] = int(all(k in n["dc_pos"] and k in n["dc_neg"] for k in both) and (False, 0) in n["dc_pos"] and
                                 (True, 0) in n["dc_pos"])
        elif wanted == "ac_all":
            counts[wanted] = int(n["ac_pos"] == set(range(1, 11)) == n["ac_neg"])
        elif wanted == "densest":
            counts[wanted] = int(n["longest_block"] == 20 + 63 * 26)
        elif wanted == "sparsest":
            counts[wanted] = int(n["shortest_block"] == 4)
        elif wanted == "one_mcu":
            counts[wanted] = int(case["mcus_per_row"] * case["mcu_rows"] == 1)
        elif wanted == "row_512":
            counts[wanted] = int(case["mcus_per_row"] == 512 and case["mcu_rows"] == 1)
        elif wanted.startswith("tail_"):
            counts[wanted] = int((8 - n["tail_bits"]) % 8 == int(wanted[5:]))
        elif wanted.startswith("blocks_"):
            counts[wanted] = int(n["blocks"] == int(wanted[7:]))
        elif wanted.startswith("bytes_"):
            counts[wanted] = int(n["unstuffed_bytes"] == int(wanted[6:]))
        elif wanted == "ff_run":
            counts[wanted] = int(n["ff_longest_run"] >= 3)
        elif wanted == "ff_chunk_edge":
            counts[wanted] = min(n["ff_last_of_chunk"], n["ff_first_of_chunk"], n["ff_both_sides_of_a_chunk_edge"])
        else:
            counts[wanted] = n[wanted]
    return counts


_CASES = None


def cases():
    """every case, its edges counted (case["edges"], case["reached"]) and asserted"""
    global _CASES
    if _CASES is None:
        made = _fixed() + [SEARCHES[name][0](SEEDS[name]) for name in SEARCHES]
        for case in made:
            case["edges"] = edges(case)
            case["reached"] = _met(case, case["edges"])
            assert all(count > 0 for count in case["reached"].values()), (case["name"], case["reached"])
        assert len(made) < 40
        _CASES = made
    return _CASES


def search(limit=200000):
    """the first seed of every searched case whose edges are met"""
    for name, (make, accept) in SEARCHES.items():
        if name in SEEDS:
            continue
        for seed in range(limit):
            case = make(seed)
            if accept(edges(case)) and all(c > 0 for c in _met(case, edges(case)).values()):
                print('    "%s": %d,' % (name, seed), flush=True)
                break
        else:
            print("    # %s: no seed below %d" % (name, limit), flush=True)


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
    else:
        for c in cases():
            print(c["name"], len(c["blocks"]), c["reached"])

/*
 * JpegWriter.h - the entropy half of the JPEG screenshot writer: quantised coefficient blocks, as the pixel stage
 * (csrc/jpeg_encode.h) leaves them, to the bytes of a baseline JPEG file.
 *
 * The file is the one the reference's encoder writes in its one-pass mode (solr/images/jpge.cpp): the markers in the
 * order of emit_markers (:517-525) - SOI, JFIF APP0, one DQT per table, SOF0, four DHT segments with the standard tables
 * of ITU T.81 annex K.3, SOS - then one interleaved scan coded as code_coefficients_pass_two does (:883-952), closed by
 * terminate_pass_two (:1032-1039).  encode is that one-pass coder.  scan makes the same entropy-coded segment in the steps of
 * csrc/jpeg_entropy.h - bits, prefix sum, emit, count, stuff - which is how the device codes it (csrc/solr_jpeg_entropy.hip)
 * and what the host-only engine runs; a file is then header + scan + EOI.
 *
 * Each of the three also writes the file of jpge's two-pass mode (params::m_two_pass_flag): the symbols of the blocks are
 * counted first (:837-881), four Huffman tables built for exactly those counts (optimize_huffman_table, :353-397;
 * csrc/jpeg_entropy.h optimiseTable) and written in the DHT segments in place of the standard ones, and the scan coded
 * with them.
 */
#pragma once

#include <string>
#include <vector>

namespace jpn
{
struct Huffman; /* csrc/jpeg_entropy.h: bits, values and the number of values of a file's four tables, in DHT order */
}

namespace solr
{
class JpegWriter
{
public:
    /* quant: the luma and the chroma table in zigzag order (jpe::quantTable); blocks: nbBlocks x 64 coefficients in
     * MCU order - the luma blocks row by row, then Cb, then Cr - each in zigzag order.  lumaH x lumaV is 1x1, 2x1 or
     * 2x2.  Returns the file's bytes.  optimise: jpge's two-pass file - a first pass counts the symbols, the tables built
     * for them are written and coded with */
    static std::vector<unsigned char> encode(int width, int height, int lumaH, int lumaV,
                                             const unsigned short quant[2][64], const short *blocks, long nbBlocks,
                                             bool optimise = false);
    /* everything encode writes in front of the entropy-coded segment: SOI ... SOS.  tables: those of the four DHT
     * segments, the standard ones when null */
    static std::vector<unsigned char> header(int width, int height, int lumaH, int lumaV,
                                             const unsigned short quant[2][64], const jpn::Huffman *tables = nullptr);
    /* the entropy-coded segment of the same blocks - stuffed, the last byte completed, no EOI - by the loops of
     * csrc/jpeg_entropy.h in the decomposed order.  false, `out` untouched, when a block is outside what the standard
     * tables code (a DC difference beyond 2047, an AC coefficient beyond 1023).  optimised not null: census and
     * optimiseTables first, the segment coded with those tables, which come back in *optimised (untouched on false) for
     * the header */
    static bool scan(int lumaH, int lumaV, const short *blocks, long nbBlocks, std::vector<unsigned char> &out,
                     jpn::Huffman *optimised = nullptr);
    static bool writeFile(const std::string &filename, const std::vector<unsigned char> &bytes);
};
}

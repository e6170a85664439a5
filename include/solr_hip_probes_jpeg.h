/*
 * solr_hip_probes_jpeg.h - test-only entry points of libsolr_hip.so for the two kernels that make the optimised Huffman
 * tables of a JPEG file (sol-r_amd/csrc/solr_jpeg_entropy.hip: k_jpegSymbolCounts, k_jpegOptimiseTables), each on its own.
 * and for the resident pipeline of JPEG frames in flight on the caller's blocks.  Not part of the product's interface.
 * All run on the device of solr_hip_get_device() on a stream of their own, with or without an initialised scene; the first
 * two give their device buffers back before they return.
 */
#ifndef SOLR_HIP_PROBES_JPEG_H
#define SOLR_HIP_PROBES_JPEG_H

#include "solr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The census: the symbols of nbBlocks (1 ... 2^24) coefficient blocks of 64 shorts in MCU and zigzag order, lumaBlocks
 * (1, 2 or 4) luma blocks per MCU, counted into counts[536] - DC luma [0, 12), DC chroma [12, 24), AC luma [24, 280), AC
 * chroma [280, 536), a DC counter per category and an AC counter per (run << 4) + size symbol, 0xF0 and 0x00 among them.
 * 0; -1 with the error set, nothing written, for arguments out of range or a block outside the domain (a DC difference
 * beyond +-2047, an AC coefficient beyond +-1023). */
int solr_hip_probe_jpeg_census(const short *coefficients, long nbBlocks, int lumaBlocks, unsigned int *counts);

/* The table builder: counts[536] laid out as above to the four tables of SolrJpegHuffman - DC luma, AC luma, DC chroma,
 * AC chroma; values behind nbValues are zero.  0, or -1 with the error set. */
int solr_hip_probe_jpeg_tables(const unsigned int *counts, SolrJpegHuffman *tables);

/* JPEG frames in flight on the caller's blocks: `coefficients` (nbBlocks * 64 shorts on the host, as
 * solr_hip_jpeg_blocks_to_scan takes them; of `source` the size and the sampling are used, the rest checked) through the
 * same slots and the same steps as solr_hip_frame_to_jpeg_async - one implementation, which differs only in where the
 * blocks come from: uploaded on a stream of the probe's own, which is waited for once (the caller's memory is pageable and
 * his again on return).  optimised != 0: with tables built for the blocks.  Returns a ticket for solr_hip_jpeg_wait, or -1
 * with the error set.  The slots stay (until reshape_scene or finalize_scene of an initialised engine). */
int solr_hip_probe_jpeg_stream_blocks(const SolrJpegSource *source, const short *coefficients, long nbBlocks, int optimised);

#ifdef __cplusplus
}
#endif
#endif

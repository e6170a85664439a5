/*
 * jpeg_device.h - what the two device halves of the JPEG writer share: solr_jpeg_encode.hip (the pixel stage) offers its
 * argument checks and its kernel on device buffers to solr_jpeg_entropy.hip (the entropy stage), so that a picture's
 * coefficients can go from one to the other without leaving the device.
 */
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/solr_hip.h"

namespace solreng
{
/* what the quantise step reads: the luma and the chroma table in zigzag order, then their reciprocals */
struct JpegEncodeTables
{
    unsigned short quant[2][64];
    unsigned recip[2][64];
};

/* The checks of solr_hip_rgb_to_jpeg_blocks on everything but the pointers, with the error set in that entry's words under
 * the name `who`; *nbBlocks receives the number of blocks the picture has.  false: refused */
bool jpegSourceAccepted(const char *who, const SolrJpegSource *source, long *nbBlocks);

/* k_jpegCoefficients on `stream`: dRgb (width * height * 3 bytes) to dCoefficients (nbBlocks * 64 shorts), both on the
 * device.  `tables` is filled here and copied to dTables (sizeof(JpegEncodeTables) bytes, 16-byte aligned) on the stream:
 * it must live until the stream has been waited for */
void launchJpegCoefficients(const SolrJpegSource &source, JpegEncodeTables &tables, JpegEncodeTables *dTables,
                            const unsigned char *dRgb, short *dCoefficients, long nbBlocks, hipStream_t stream);
/* The same for a caller that does not wait (solr_hip_frame_to_jpeg_async): the tables travel to dTables as a kernel's
 * argument (k_jpegPutTables), so nothing of the host's has to outlive the call */
void launchJpegCoefficientsResident(const SolrJpegSource &source, JpegEncodeTables *dTables, const unsigned char *dRgb,
                                    short *dCoefficients, long nbBlocks, hipStream_t stream);
/* ... and the caller counts the blocks (solr_hip_jpeg_encoded_blocks) once the call they were made for has delivered: a
 * call that only found out how large its result is, and is made again with room for it, counts once */
void countJpegEncodedBlocks(long nbBlocks);
}

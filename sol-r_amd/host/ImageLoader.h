/*
 * ImageLoader.h - texture files: 24-bit BMP, TGA (types 2 and 10) and baseline / extended-sequential JPEG.
 *
 * Takes the place of the reference's solr::ImageLoader with its jpgd / tgad decoders (reference:
 * solr/images/ImageLoader.cpp:69-320, jpgd.cpp, tgad.cpp) behind GPUKernel::loadTextureFromFile.  The readers fill an
 * Image and never touch a texture slot: the caller replaces the slot only when a file loaded.  Every length and index
 * read from a file is checked against the file's size; a bad file gives false and a reason, never an exception.
 *
 * A JPEG file is read in two steps, because its second half is device work: parseJPEG reads the markers and decodes the
 * Huffman stream into coefficient blocks, and the pixel stage (csrc/jpeg_pixels.h) turns those into RGB bytes - on the
 * CPU through jpegPixelsOnHost, on the device through solr_hip_jpeg_to_rgb (GPUKernel::jpegPixels chooses).
 */
#pragma once

#include <string>
#include <vector>

#include "../../include/solr_hip.h"

namespace solr
{
struct Image
{
    int width = 0, height = 0, depth = 0; /* depth: bytes per pixel, 3 or 4 */
    std::vector<unsigned char> pixels;    /* width * height * depth, as the texture slot keeps them */
};

class ImageLoader
{
public:
    /* reference: ImageLoader.cpp:69-164.  Rows in file order, BGR swapped to RGB, depth 3.  Deviation: the header is
     * read by its on-disk layout (the reference's Linux build reads it through a struct with 8-byte `unsigned long`
     * fields and so cannot load a BMP at all), the pixels from bfOffBits, and each row's padding to 4 bytes is skipped */
    static bool loadBMP24(const std::string &filename, Image &image, std::string &why);
    /* reference: tgad.cpp:23-337 through ImageLoader.cpp:288-311.  Pixels in file order, BGR swapped to RGB, the
     * fourth byte of 32-bit files kept */
    static bool loadTGA(const std::string &filename, Image &image, std::string &why);
    /* SOF0 / SOF1, 8 bit, three components in one interleaved scan, luma 1x1, 2x1 or 2x2 with chroma 1x1.
     * coefficients: frame.mcusPerRow * frame.mcuRows * (lumaH * lumaV + 2) blocks of 64, see include/solr_hip.h */
    static bool parseJPEG(const std::string &filename, SolrJpegFrame &frame, std::vector<short> &coefficients,
                          std::string &why);
    /* the pixel stage in a loop over the MCUs; rgb: width * height * 3 bytes, turned by 180 degrees */
    static void jpegPixelsOnHost(const SolrJpegFrame &frame, const short *coefficients, unsigned char *rgb);
};
}

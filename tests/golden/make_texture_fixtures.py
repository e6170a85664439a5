"""Generates tests/golden/texture_files.npz and, where they are missing, the small image files under
tests/golden/textures/ that tests/test_texture_files.py and tests/test_texture_files_gpu.py load.

Run where the reference's tree exists (SOLR_REFERENCE, default /root/reference):

    python tests/golden/make_texture_fixtures.py

What the texture loader is held to is THE REFERENCE'S OWN decoders: the script compiles the reference's
solr/images/jpgd.cpp and tgad.cpp with a few lines of driver into a temporary directory outside the repository,
decodes every input file with them and keeps one expected array per file:

    *.jpg   jpgd's decompress_jpeg_image_from_file(..., req_comps = 3), turned by 180 degrees as the reference's
            ImageLoader::loadJPEG stores it (ImageLoader.cpp:170-190): decoded[::-1, ::-1, :]
    *.tga   the buffer LoadTGA fills (tgad.cpp), (height, width, 3 or 4)
    *.bmp   derived here from the file's bytes with numpy, independently of the loader: rows in file order without
            their padding, BGR swapped to RGB (the reference's own loader reads the header through a struct whose
            fields are 8 bytes wide on Linux and cannot be run)

PIL / libjpeg is not the yardstick (it differs from jpgd by several levels); it only writes the input
files.  Files that must be refused (progressive, grayscale) get no array.  Data only: nothing compiled and none of the
reference's source is written into the repository."""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TEXTURES = os.path.join(HERE, "textures")
REFERENCE = os.environ.get("SOLR_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "texture_files.npz")

REFERENCE_TEXTURES = ["0220r.jpg", "0100d.jpg"]          # 4:2:0 and 4:4:4, both 512x512
REFUSED = ["progressive_24x24.jpg", "gray_19x13.jpg"]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "jpgd.h"
#include "tgad.h"
int main(int argc, char **argv)
{
    if (argc != 4)
        return 2;
    int width = 0, height = 0, depth = 0;
    unsigned char *pixels = 0;
    if (!strcmp(argv[1], "jpg"))
    {
        int actual = 0;
        pixels = jpgd::decompress_jpeg_image_from_file(argv[2], &width, &height, &actual, 3);
        depth = 3;
    }
    else
    {
        Texture texture;
        memset(&texture, 0, sizeof(texture));
        if (LoadTGA(&texture, argv[2]))
        {
            pixels = texture.imageData;
            width = texture.width;
            height = texture.height;
            depth = texture.bpp / 8;
        }
    }
    if (!pixels)
        return 1;
    FILE *out = fopen(argv[3], "wb");
    int header[3] = {width, height, depth};
    fwrite(header, sizeof(header), 1, out);
    fwrite(pixels, 1, (size_t)width * height * depth, out);
    fclose(out);
    return 0;
}
"""


def picture(width, height, seed, saturated=False):
    """smooth ramps, noise, and - with `saturated` - full primaries with hard edges between them"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    a = np.stack([255 * x / max(width - 1, 1), 255 * y / max(height - 1, 1),
                  127 + 127 * np.sin(x / 3.0 + y / 5.0)], axis=-1)
    a += rng.normal(0, 24, a.shape)
    if saturated:
        primaries = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [255, 255, 0],
                              [0, 255, 255], [255, 0, 255]], np.float64)
        cells = rng.randint(0, len(primaries), ((height + 3) // 4, (width + 3) // 4))
        blocks = primaries[np.repeat(np.repeat(cells, 4, axis=0), 4, axis=1)[:height, :width]]
        mask = (x + y) % 8 < 5
        a[mask] = blocks[mask]
    return np.clip(a, 0, 255).astype(np.uint8)


def write_inputs():
    """the committed inputs; only files that are missing are written (PIL is needed for the JPEG ones)"""
    os.makedirs(TEXTURES, exist_ok=True)

    def missing(name):
        return not os.path.exists(os.path.join(TEXTURES, name))

    jpegs = {
        "444_24x17.jpg": (picture(24, 17, 1), dict(quality=92, subsampling=0)),
        "444_16x16_q100.jpg": (picture(16, 16, 2, saturated=True), dict(quality=100, subsampling=0)),
        "444_8x8_flat.jpg": (np.full((8, 8, 3), (200, 60, 30), np.uint8), dict(quality=90, subsampling=0)),
        "422_33x9.jpg": (picture(33, 9, 3), dict(quality=60, subsampling=1)),
        "420_37x21.jpg": (picture(37, 21, 4, saturated=True), dict(quality=75, subsampling=2)),
        "420_31x31_optimized.jpg": (picture(31, 31, 5), dict(quality=50, subsampling=2, optimize=True)),
        "420_40x40_restart2.jpg": (picture(40, 40, 6, saturated=True),
                                   dict(quality=80, subsampling=2, restart_marker_blocks=2)),
        "progressive_24x24.jpg": (picture(24, 24, 7), dict(quality=80, subsampling=0, progressive=True)),
    }
    if any(missing(n) for n in list(jpegs) + ["gray_19x13.jpg"]):
        from PIL import Image
        for name, (pixels, options) in jpegs.items():
            if missing(name):
                Image.fromarray(pixels).save(os.path.join(TEXTURES, name), "JPEG", **options)
        if missing("gray_19x13.jpg"):
            Image.fromarray(picture(19, 13, 8)[..., 0]).save(os.path.join(TEXTURES, "gray_19x13.jpg"), "JPEG", quality=80)

    for name in REFERENCE_TEXTURES:
        if missing(name):
            shutil.copyfile(os.path.join(REFERENCE, "medias", "textures", name), os.path.join(TEXTURES, name))

    def bmp(name, pixels):
        h, w, _ = pixels.shape
        row = (w * 3 + 3) & ~3
        body = b"".join(pixels[y, :, ::-1].tobytes() + b"\xAA" * (row - w * 3) for y in range(h))
        info = struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(body), 2835, 2835, 0, 0)
        head = struct.pack("<2sIHHI", b"BM", 14 + len(info) + len(body), 0, 0, 14 + len(info))
        with open(os.path.join(TEXTURES, name), "wb") as f:
            f.write(head + info + body)

    if missing("rgb_6x5.bmp"):
        bmp("rgb_6x5.bmp", picture(6, 5, 9, saturated=True))       # 18 bytes a row: 2 bytes of padding
    if missing("rgb_8x4.bmp"):
        bmp("rgb_8x4.bmp", picture(8, 4, 10))                       # 24 bytes a row: none

    def tga(name, pixels, rle):
        h, w, d = pixels.shape
        bgr = pixels.copy()
        bgr[..., 0], bgr[..., 2] = pixels[..., 2], pixels[..., 0]
        flat = bgr.reshape(-1, d)
        head = struct.pack("<BBBHHBHHHHBB", 0, 0, 10 if rle else 2, 0, 0, 0, 0, 0, w, h, 8 * d, 0)
        body = b""
        if not rle:
            body = flat.tobytes()
        else:
            i = 0
            while i < len(flat):
                run = 1
                while i + run < len(flat) and run < 128 and (flat[i + run] == flat[i]).all():
                    run += 1
                if run > 1:
                    body += bytes([127 + run]) + flat[i].tobytes()
                    i += run
                    continue
                raw = 1
                while i + raw < len(flat) and raw < 128 and not (flat[i + raw] == flat[i + raw - 1]).all():
                    raw += 1
                body += bytes([raw - 1]) + flat[i:i + raw].tobytes()
                i += raw
        with open(os.path.join(TEXTURES, name), "wb") as f:
            f.write(head + body)

    def flat_areas(pixels):
        pixels[1:3, 1:6] = pixels[1, 1]        # runs, also across the end of a row
        pixels[-1, :] = pixels[-1, 0]
        return pixels

    if missing("raw24_7x5.tga"):
        tga("raw24_7x5.tga", picture(7, 5, 11), rle=False)
    if missing("rle24_7x5.tga"):
        tga("rle24_7x5.tga", flat_areas(picture(7, 5, 12)), rle=True)
    if missing("rle32_9x3.tga"):
        rgba = np.concatenate([picture(9, 3, 13), picture(9, 3, 14)[..., :1]], axis=-1)
        tga("rle32_9x3.tga", flat_areas(rgba), rle=True)

    if missing("quad.mtl"):
        with open(os.path.join(TEXTURES, "quad.mtl"), "w") as f:
            f.write("newmtl picture\nKd 1.0 1.0 1.0\nKs 0.1 0.1 0.0\nillum 2\nmap_Kd 444_24x17.jpg\n")
    if missing("quad.obj"):
        with open(os.path.join(TEXTURES, "quad.obj"), "w") as f:
            f.write("mtllib quad.mtl\n"
                    "v -1.0 -1.0 0.0\nv 1.0 -1.0 0.0\nv 1.0 1.0 0.0\nv -1.0 1.0 0.0\n"
                    "vt 0.0 0.0\nvt 1.0 0.0\nvt 1.0 1.0\nvt 0.0 1.0\n"
                    "vn 0.0 0.0 1.0\n"
                    "usemtl picture\nf 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3/1 4/4/1\n")


def build_decoder(tmp):
    images = os.path.join(REFERENCE, "solr", "images")
    with open(os.path.join(tmp, "driver.cpp"), "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "decode")
    subprocess.run(["g++", "-O1", "-w", "-I", images, "-o", exe, os.path.join(tmp, "driver.cpp"),
                    os.path.join(images, "jpgd.cpp"), os.path.join(images, "tgad.cpp")], check=True)
    return exe


def decode(exe, tmp, kind, path):
    out = os.path.join(tmp, "pixels.bin")
    if subprocess.run([exe, kind, path, out], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode != 0:
        return None
    raw = open(out, "rb").read()
    w, h, d = struct.unpack("<3i", raw[:12])
    return np.frombuffer(raw[12:], np.uint8).reshape(h, w, d).copy()


def bmp_expected(path):
    raw = np.fromfile(path, np.uint8)
    off_bits = int(raw[10:14].view("<u4")[0])
    w, h = (int(v) for v in raw[18:26].view("<i4"))
    row = (w * 3 + 3) & ~3
    rows = raw[off_bits:off_bits + row * h].reshape(h, row)[:, :w * 3].reshape(h, w, 3)
    return np.ascontiguousarray(rows[..., ::-1])


def main():
    write_inputs()
    expected = {}
    tmp = tempfile.mkdtemp(prefix="texture_fixtures_")
    try:
        exe = build_decoder(tmp)
        for name in sorted(os.listdir(TEXTURES)):
            path = os.path.join(TEXTURES, name)
            if name in REFUSED:
                continue
            if name.endswith(".jpg"):
                decoded = decode(exe, tmp, "jpg", path)
                assert decoded is not None, name
                expected[name] = np.ascontiguousarray(decoded[::-1, ::-1, :])
            elif name.endswith(".tga"):
                expected[name] = decode(exe, tmp, "tga", path)
                assert expected[name] is not None, name
            elif name.endswith(".bmp"):
                expected[name] = bmp_expected(path)
    finally:
        shutil.rmtree(tmp)
    np.savez_compressed(OUT, **expected)
    for name, a in expected.items():
        print("%-28s %s" % (name, a.shape))
    print("%s: %d arrays, %d bytes" % (OUT, len(expected), os.path.getsize(OUT)))


if __name__ == "__main__":
    sys.exit(main())

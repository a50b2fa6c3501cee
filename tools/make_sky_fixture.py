"""Decode the reference's sky environment map into the raw texture fixture.

Run once in the build container (it reads /root/reference, which does not exist on
the GPU box):  python tools/make_sky_fixture.py

What it reproduces (reference behaviour, not a fix):
  * textures.cu:15-17   cv::imread (BGR) + cvtColor(BGR2RGBA)  -> RGBA8, alpha = 255.
                        PIL decodes the 8-bit RGB PNG losslessly to the same bytes.
  * textures.cu:32-33   cudaMemcpy2DToArray(..., width*sizeof(uint8_t), height, ...)
                        copies only `width` BYTES per row = width/4 texels, so only
                        columns [0, width/4) of the cudaArray hold image data.  We keep
                        exactly those columns; the renderer treats the rest as zero.

Output: assets/sky.cptex  (format: see cpppathtracer_amd/texture_io.py / include/cpt.h)
"""
import os
import struct
import sys

import numpy as np

REF_PNG = "/root/reference/textures/sky.png"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets", "sky.cptex")


def fixture_bytes(png_path: str = REF_PNG, width: int = None) -> bytes:
    """The .cptex file's bytes for the PNG at `png_path` (header + the W/4 valid columns as
    RGBA8).  `width`: the texture's logical width W when the PNG holds only those W/4 columns
    (tests/golden/sky_valid_columns.png, written by valid_columns_png below; its pixels are the
    reference PNG's, re-encoded losslessly).  tests/test_sky_fixture.py re-runs this on that PNG
    and compares it with the committed assets/sky.cptex byte for byte."""
    from PIL import Image

    img = Image.open(png_path)
    assert img.mode == "RGB", img.mode
    rgb = np.asarray(img, dtype=np.uint8)  # (H, W, 3), or (H, W/4, 3) with `width`
    h, w, _ = rgb.shape
    if width is not None:
        assert w == width // 4, (w, width)
        w = width
    valid_cols = w // 4  # textures.cu:32-33 quirk: width bytes, not width texels
    rgba = np.empty((h, valid_cols, 4), dtype=np.uint8)
    rgba[..., :3] = rgb[:, :valid_cols, :]
    rgba[..., 3] = 255
    # header: magic, logical width, height, stored (valid) columns, reserved
    hdr = b"CPTTEX01" + struct.pack("<IIII", w, h, valid_cols, 0)
    return hdr + np.ascontiguousarray(rgba).tobytes()


def valid_columns_png(out_path: str, png_path: str = REF_PNG) -> None:
    """The W/4 columns of the PNG that the upload reads, as a PNG of their own (the test fixture:
    the whole image is larger than a committed file may be)."""
    from PIL import Image

    rgb = np.asarray(Image.open(png_path), dtype=np.uint8)
    Image.fromarray(np.ascontiguousarray(rgb[:, : rgb.shape[1] // 4, :])).save(out_path, optimize=True)


def main() -> int:
    data = fixture_bytes(REF_PNG)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT}: {len(data)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())

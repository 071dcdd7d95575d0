"""A PNG writer and reader for 8-bit RGB images, with zlib and struct only: what the colour path needs to leave a picture a
person can open.  Every scanline is written with filter type 0 (None); ``read_png`` reads files of that kind."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(img) -> bytes:
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png takes a uint8 [H, W, 3] image, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)              # filter byte 0, then the row's RGB bytes
    rows[:, 1:] = a.reshape(h, 3 * w)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)          # 8 bits, colour type 2 (RGB), deflate, adaptive filtering, no interlace
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b"")


def write_png(path: str, img) -> None:
    """img: uint8 [H, W, 3] (numpy, or anything np.asarray takes) -> an 8-bit RGB PNG at `path`."""
    data = encode_png(img)
    with open(path, "wb") as f:
        f.write(data)


def read_png(path: str) -> np.ndarray:
    """The uint8 [H, W, 3] image of an 8-bit RGB, non-interlaced PNG whose scanlines all use filter 0; anything else raises
    ValueError, as does a wrong CRC."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != SIGNATURE:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, head, ended = 8, [], None, False
    while pos + 12 <= len(buf):
        n, kind = struct.unpack(">I4s", buf[pos:pos + 8])
        data = buf[pos + 8:pos + 8 + n]
        if len(data) != n or pos + 12 + n > len(buf):
            raise ValueError(f"{path}: chunk {kind!r} is cut short")
        if struct.unpack(">I", buf[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + data) & 0xFFFFFFFF):
            raise ValueError(f"{path}: chunk {kind!r} has a wrong CRC")
        pos += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif kind == b"IDAT":
            idat.append(data)
        elif kind == b"IEND":
            ended = True
            break
    if head is None or not ended:
        raise ValueError(f"{path}: IHDR or IEND is missing")
    w, h, depth, colour, comp, filt, lace = head
    if (depth, colour, comp, filt, lace) != (8, 2, 0, 0, 0):
        raise ValueError(f"{path}: only 8-bit RGB, non-interlaced PNGs are read (got depth {depth}, colour type {colour}, interlace {lace})")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != h * (1 + 3 * w):
        raise ValueError(f"{path}: {raw.size} bytes of image data for {w} x {h}")
    rows = raw.reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError(f"{path}: a scanline uses a filter other than 0")
    return rows[:, 1:].reshape(h, w, 3).copy()

"""Writer of the one HDF5 form the reference's data scripts produce: MATLAB's ``h5create(f, '/X', size(X), 'Datatype', 'single');
h5write(f, '/X', single(X))`` (Generate_Data_for_Training.m:74-78, Generate_Data_for_Test.m:73-77).  That is

  * superblock version 0 (8-byte offsets and lengths), the root group as a symbol table: a version-1 group B-tree with one
    symbol-table node (SNOD) and a local heap holding the names;
  * one version-1 object header per dataset: dataspace (version 1, fixed maximum dimensions), IEEE float32 little-endian
    datatype, fill-value message, contiguous layout (version 3);
  * the data stored contiguously, dimensions reversed: MATLAB writes its column-major matrix M[r, c] as an HDF5 dataset of shape
    (c, r), so a C-order reader (h5py, lft_amd.h5lite) sees M transposed.

``write_sai_pair(path, lr, hr)`` takes the two mosaics in the MATLAB matrix orientation (what lft_amd.prepare returns) and writes
them in that form; lft_amd.h5lite reads them back.  Nothing else of HDF5 is written here (h5lite.File stays read-only).
"""
from __future__ import annotations

import struct
from typing import List, Sequence, Tuple

import numpy as np

SIGNATURE = b"\x89HDF\r\n\x1a\n"
UNDEF = (1 << 64) - 1
GROUP_LEAF_K, GROUP_INTERNAL_K = 4, 16            # libhdf5's defaults: an SNOD holds 2*4 entries, a B-tree node 2*16 children


def _pad8(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 8)


def _message(mtype: int, body: bytes, flags: int = 0) -> bytes:
    body = _pad8(body)
    return struct.pack("<HHB3x", mtype, len(body), flags) + body


def _object_header(messages: Sequence[bytes]) -> bytes:
    """Version-1 object header: 12-byte prefix padded to 16, then the messages (each 8-byte aligned)."""
    body = b"".join(messages)
    return struct.pack("<BBHII4x", 1, 0, len(messages), 1, len(body)) + body


def _dataset_header(shape: Tuple[int, ...], data_addr: int, nbytes: int) -> bytes:
    rank = len(shape)
    dataspace = struct.pack("<BBBB4x", 1, rank, 1, 0) + struct.pack(f"<{rank}Q", *shape) + struct.pack(f"<{rank}Q", *shape)
    # floating point, version 1; bit field: little-endian, implied mantissa msb (normalization 2), sign at bit 31; 4 bytes;
    # properties: offset 0, precision 32, exponent at 23 of 8 bits, mantissa at 0 of 23 bits, bias 127
    datatype = struct.pack("<B3BI", 0x11, 0x20, 31, 0, 4) + struct.pack("<HHBBBBI", 0, 32, 23, 8, 0, 23, 127)
    fill = struct.pack("<BBBB", 2, 2, 2, 0)            # version 2, allocation late, write fill never, no fill value defined
    layout = struct.pack("<BBQQ", 3, 1, data_addr, nbytes)
    return _object_header([_message(0x0001, dataspace), _message(0x0003, datatype, flags=1), _message(0x0005, fill, flags=1),
                           _message(0x0008, layout)])


def write_datasets(path: str, datasets: Sequence[Tuple[str, np.ndarray]], userblock: int = 0) -> None:
    """Write float32 arrays as root datasets, each stored with exactly the shape given (C order).  The caller reverses the
    dimensions (``write_sai_pair`` does).  At most 2 * GROUP_LEAF_K datasets: one symbol-table node.  ``userblock`` (0 or
    512 * 2^n bytes, zero-filled) goes in front of the superblock, as in a MATLAB -v7.3 file; addresses are relative to it."""
    if userblock and (userblock < 512 or userblock & (userblock - 1)):
        raise ValueError(f"user block of {userblock} bytes: 0 or a power of two >= 512")
    if not 1 <= len(datasets) <= 2 * GROUP_LEAF_K:
        raise ValueError(f"{len(datasets)} datasets: this writer holds 1 .. {2 * GROUP_LEAF_K} in the root group")
    arrays = [(str(n), np.ascontiguousarray(a, dtype="<f4")) for n, a in datasets]
    names = [n for n, _ in arrays]
    if len(set(names)) != len(names) or any(not n or "/" in n or "\0" in n for n in names):
        raise ValueError(f"dataset names must be distinct plain names, got {names}")

    # local heap data segment: "" at offset 0 (the root's own name), then every name, 8-byte aligned
    heap_data, name_off = bytearray(8), {}
    for n in names:
        name_off[n] = len(heap_data)
        heap_data += _pad8(n.encode() + b"\0")

    # layout: superblock | root header | B-tree node | local heap header + data | SNOD | dataset headers | data
    SB = 96
    root_hdr_len = len(_object_header([_message(0x0011, bytes(16))]))
    btree_len = 8 + 16 + 2 * GROUP_INTERNAL_K * 8 + (2 * GROUP_INTERNAL_K + 1) * 8
    heap_len = 32 + len(heap_data)
    snod_len = 8 + 2 * GROUP_LEAF_K * 40
    a_root = SB
    a_btree = a_root + root_hdr_len
    a_heap = a_btree + btree_len
    a_snod = a_heap + heap_len
    a = a_snod + snod_len
    ds_addr, hdr_lens = [], [len(_dataset_header(arr.shape, 0, 0)) for _, arr in arrays]
    for ln in hdr_lens:
        ds_addr.append(a)
        a += ln
    data_addr = []
    for _, arr in arrays:
        a += -a % 8
        data_addr.append(a)
        a += arr.nbytes
    eof = a

    out = bytearray(eof)                                         # relative addresses; the user block is prepended at the end
    # superblock 0 with the root group's symbol-table entry (cache type 1: B-tree and heap addresses in the scratch pad)
    sb = SIGNATURE + struct.pack("<8B", 0, 0, 0, 0, 0, 8, 8, 0) + struct.pack("<HHI", GROUP_LEAF_K, GROUP_INTERNAL_K, 0)
    sb += struct.pack("<4Q", userblock, UNDEF, eof, UNDEF)
    sb += struct.pack("<QQI4xQQ", 0, a_root, 1, a_btree, a_heap)
    assert len(sb) == SB
    out[0:SB] = sb
    out[a_root:a_root + root_hdr_len] = _object_header([_message(0x0011, struct.pack("<QQ", a_btree, a_heap))])
    # group B-tree, one leaf: key 0 = "" , child = the SNOD, key 1 = the greatest name in it
    order = sorted(range(len(names)), key=lambda i: names[i].encode())
    bt = b"TREE" + struct.pack("<BBH", 0, 0, 1) + struct.pack("<QQ", UNDEF, UNDEF)
    bt += struct.pack("<QQQ", 0, a_snod, name_off[names[order[-1]]])
    out[a_btree:a_btree + len(bt)] = bt
    out[a_heap:a_heap + 32] = b"HEAP" + struct.pack("<B3xQQQ", 0, len(heap_data), 1, a_heap + 32)   # free list: 1 = none (libhdf5)
    out[a_heap + 32:a_heap + heap_len] = heap_data
    sn = b"SNOD" + struct.pack("<BBH", 1, 0, len(names))
    for i in order:                                              # entries sorted by name, cache type 0
        sn += struct.pack("<QQI4x16x", name_off[names[i]], ds_addr[i], 0)
    out[a_snod:a_snod + len(sn)] = sn
    for (n, arr), ah, ad in zip(arrays, ds_addr, data_addr):
        h = _dataset_header(arr.shape, ad, arr.nbytes)
        out[ah:ah + len(h)] = h
        out[ad:ad + arr.nbytes] = arr.tobytes()
    with open(path, "wb") as f:
        f.write(bytes(userblock))
        f.write(out)


def write_sai_pair(path: str, lr, hr, hr_first: bool = False) -> None:
    """One sample file of the data scripts: ``Lr_SAI_y`` and ``Hr_SAI_y`` given in the MATLAB matrix orientation (2-D numpy arrays or
    tensors), stored with reversed dimensions.  The training script writes Lr first, the test script Hr first (``hr_first``)."""
    def host(x) -> np.ndarray:
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        if x.ndim != 2:
            raise ValueError(f"expected a 2-D mosaic, got shape {x.shape}")
        return x.astype(np.float32, copy=False).T
    pair: List[Tuple[str, np.ndarray]] = [("Lr_SAI_y", host(lr)), ("Hr_SAI_y", host(hr))]
    write_datasets(path, pair[::-1] if hr_first else pair)

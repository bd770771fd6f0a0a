"""Slabs of an EBCK chunk container.

`ebcc_encode_chunking` / `ebcc_encode_chunking_compat` (include/ebcc_codec.h) cut every frame of a (nt, H, W) array into
spatial chunks - 1024 x 1024 by default, edge chunks padded - and store them as one container: an 80-byte header, then per
chunk `u64 nbytes | EBCC stream` in C order of chunk index (ebcc_amd/sharding.py writes the same layout).  The reference's
only read of such a container is `ebcc_decode_chunking`: every chunk of every time step.  `read_slab` decodes a sub-array
instead: only the chunks it meets are read, of those only the code-blocks it depends on are decoded, and every chunk's part
goes straight to its place in the result (include/ebcc_hip.h: placed boxes).  The result is bit for bit
`decode_chunking(buf)[t, rows, cols]`.

`encode_resident` is the write side for an array that lies on the device: the container `ebcc_encode_chunking` (or, with
`compat`, `ebcc_encode_chunking_compat`, global range included) gives for the same array on the host, byte for byte, with the
padded chunks gathered on the device (include/ebcc_hip.h: container encode from the device).

Only numpy and ctypes are needed.
"""
import ctypes

import numpy as np

from . import load


class Slab(ctypes.Structure):
    """ebcc_hip_slab, include/ebcc_hip.h"""
    _fields_ = [(n, ctypes.c_size_t) for n in ("t0", "row0", "col0", "nt", "rows", "cols")]


def _lib():
    lib = load()
    lib.ebcc_hip_last_error.restype = ctypes.c_char_p
    lib.ebcc_hip_container_info.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    lib.ebcc_hip_decode_container_slab_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Slab), ctypes.c_void_p]
    lib.ebcc_decode_chunking_slab.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Slab), ctypes.POINTER(ctypes.c_void_p)]
    lib.ebcc_decode_chunking_slab.restype = ctypes.c_size_t
    lib.ebcc_decode_chunking.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    lib.ebcc_decode_chunking.restype = ctypes.c_size_t
    lib.free_buffer.argtypes = [ctypes.c_void_p]
    lib.ebcc_hip_container_plan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    lib.ebcc_hip_encode_container.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.POINTER(ctypes.c_size_t)]
    return lib


def _bytes(buf):
    """the container as a ctypes buffer the library may read (it is never written)"""
    b = buf if isinstance(buf, bytes) else bytes(buf)
    return b, ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)


def info(buf):
    """(dims, chunk_dims) of an EBCK container, two tuples of three ints; ValueError for anything else, or a container whose
    header or chain of chunk entries is damaged"""
    lib = _lib()
    b, p = _bytes(buf)
    dims, chunk_dims = (ctypes.c_size_t * 3)(), (ctypes.c_size_t * 3)()
    if lib.ebcc_hip_container_info(p, len(b), dims, chunk_dims):
        raise ValueError((lib.ebcc_hip_last_error() or b"not an EBCK container").decode())
    return tuple(int(v) for v in dims), tuple(int(v) for v in chunk_dims)


def _range(s, n, what):
    """a slice of step 1 (or None: everything) over an axis of n -> (first, count)"""
    if s is None:
        return 0, n
    if not isinstance(s, slice):
        raise ValueError(f"{what} must be a slice or None")
    lo, hi, step = s.indices(n)
    if step != 1:
        raise ValueError(f"{what}: only slices of step 1")
    if hi <= lo:
        raise ValueError(f"{what}: the slice {s} of an axis of {n} is empty")
    return lo, hi - lo


def decode_chunking(buf):
    """the whole array of a container, (nt, H, W) float32: ebcc_decode_chunking"""
    lib = _lib()
    dims, _ = info(buf)
    b, p = _bytes(buf)
    out = ctypes.c_void_p()
    n = lib.ebcc_decode_chunking(p, len(b), ctypes.byref(out))
    if n != dims[0] * dims[1] * dims[2]:
        raise RuntimeError("ebcc_decode_chunking failed")
    a = np.frombuffer(ctypes.string_at(out.value, 4 * n), np.float32).reshape(dims).copy()
    lib.free_buffer(out)
    return a


def read_slab(buf, t=None, rows=None, cols=None, out=None, codec=None):
    """buf[t, rows, cols] of the array an EBCK container of one-frame chunks holds: `t`, `rows`, `cols` are slices of step 1
    (None: the whole axis) -> (nt, rows, cols) float32, equal bit for bit to decode_chunking(buf)[t, rows, cols].  `out`: a
    C-contiguous float32 array of that size to decode into.  `codec`: a h5_batch.BatchCodec of the chunk geometry to run on
    (any capacity); without one the engines the library keeps for ebcc_decode_chunking are used.  ValueError for slices that
    are empty, stepped or not a slice, and for data that is not such a container; RuntimeError for what the decode reports."""
    lib = _lib()
    dims, chunk_dims = info(buf)
    (t0, nt), (r0, nr), (c0, nc) = _range(t, dims[0], "t"), _range(rows, dims[1], "rows"), _range(cols, dims[2], "cols")
    if chunk_dims[0] != 1:
        raise ValueError(f"chunks of {chunk_dims[0]} frames are not supported: one-frame chunks only")
    slab = Slab(t0, r0, c0, nt, nr, nc)
    b, p = _bytes(buf)
    if out is not None and not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.size == nt * nr * nc):
        raise ValueError(f"out must be a C-contiguous float32 array of {nt * nr * nc} elements")
    if codec is not None:
        if (codec.h, codec.w) != chunk_dims[1:]:
            raise ValueError(f"the codec's frames are {codec.h} x {codec.w}, the container's chunks {chunk_dims[1]} x {chunk_dims[2]}")
        if out is None:
            out = np.empty((nt, nr, nc), np.float32)
        if lib.ebcc_hip_decode_container_slab_host(codec.ctx, p, len(b), ctypes.byref(slab), out.ctypes.data):
            raise RuntimeError("ebcc_hip_decode_container_slab_host: " + (lib.ebcc_hip_last_error() or b"?").decode())
        return out.reshape(nt, nr, nc)
    res = ctypes.c_void_p()
    n = lib.ebcc_decode_chunking_slab(p, len(b), ctypes.byref(slab), ctypes.byref(res))
    if n != nt * nr * nc:
        raise RuntimeError("ebcc_decode_chunking_slab: " + (lib.ebcc_hip_last_error() or b"?").decode())
    got = np.frombuffer(ctypes.string_at(res.value, 4 * n), np.float32).reshape(nt, nr, nc)
    lib.free_buffer(res)
    if out is None:
        return got.copy()
    out.reshape(nt, nr, nc)[...] = got
    return out.reshape(nt, nr, nc)


def plan(cfg, compat=False):
    """(chunk_dims, n_chunks) `ebcc_encode_chunking` (compat: `ebcc_encode_chunking_compat`) would use for cfg.dims /
    cfg.chunk_dims - cfg: a h5_batch.CodecConfig; all-zero chunk_dims stand for the entry point's default.  ValueError for
    what those refuse.  Host logic, no device."""
    lib = _lib()
    chunk_dims, n = (ctypes.c_size_t * 3)(), ctypes.c_size_t()
    if lib.ebcc_hip_container_plan(ctypes.byref(cfg), int(bool(compat)), chunk_dims, ctypes.byref(n)):
        raise ValueError((lib.ebcc_hip_last_error() or b"?").decode())
    return tuple(int(v) for v in chunk_dims), int(n.value)


def encode_resident(ptr, dims, cfg, codec, compat=False):
    """The EBCK container of a (nt, H, W) float32 array that lies on the device -> bytes, equal byte for byte to
    `ebcc_encode_chunking` (compat: `ebcc_encode_chunking_compat`) of the same array on the host.  `ptr`: the array's device
    address as an int, or an object with `data_ptr()` (a contiguous torch tensor on the codec's device); 4-byte alignment is
    enough.  `dims`: the array's shape.  `cfg`: a h5_batch.CodecConfig with the codec parameters and chunk_dims (its dims are
    taken from `dims`).  `codec`: a h5_batch.BatchCodec of the chunk geometry `plan` gives, any capacity.  ValueError for what
    the call refuses or NaN / Inf in the array, RuntimeError for what the encode reports."""
    lib = _lib()
    c = type(cfg).from_buffer_copy(cfg)
    c.dims[:] = [int(v) for v in dims]
    address = int(ptr.data_ptr()) if hasattr(ptr, "data_ptr") else int(ptr)
    chunk_dims, _ = plan(c, compat)
    if chunk_dims[0] != 1:
        raise ValueError(f"chunks of {chunk_dims[0]} frames are not supported: one-frame chunks only")
    if (codec.h, codec.w) != chunk_dims[1:]:
        raise ValueError(f"the codec's frames are {codec.h} x {codec.w}, the chunks {chunk_dims[1]} x {chunk_dims[2]}")
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    rc = lib.ebcc_hip_encode_container(codec.ctx, address, ctypes.byref(c), int(bool(compat)), ctypes.byref(out), ctypes.byref(n))
    if rc:
        raise (ValueError if rc == 2 else RuntimeError)("ebcc_hip_encode_container: " + (lib.ebcc_hip_last_error() or b"?").decode())
    buf = ctypes.string_at(out.value, n.value)
    lib.free_buffer(out)
    return buf

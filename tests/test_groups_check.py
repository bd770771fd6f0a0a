"""ebcc_hip_groups_check (include/ebcc_hip.h): the host-side check of a list of frame groups - the total number of frames of a
good list, -1 with a message for everything the group encode calls refuse before they touch a device.  No GPU: the pointers
are dummies, nothing is dereferenced."""
import ctypes

from tests import _lib as L

H, W = 70, 100
DUMMY = 0x1000                                                        # non-null, 4-byte aligned, never read


class FrameGroup(ctypes.Structure):
    """ebcc_hip_frame_group"""
    _fields_ = [("frames", ctypes.c_void_p), ("n_frames", ctypes.c_size_t), ("config", L.CodecConfig), ("range_of_group", ctypes.c_int)]


def lib():
    p = L.product()
    p.ebcc_hip_groups_check.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(FrameGroup), ctypes.c_size_t]
    p.ebcc_hip_groups_check.restype = ctypes.c_long
    return p


def error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


def table(items):
    """items: (pointer, frames, dims) per group"""
    t = (FrameGroup * max(1, len(items)))()
    for g, (ptr, n, dims) in enumerate(items):
        t[g].frames, t[g].n_frames = ptr, n
        t[g].config = L.make_config(dims, base_cr=10.0 + g, error=0.01, residual_type=g % 3)
        t[g].range_of_group = g & 1
    return t


GOOD = [(DUMMY, 3, (1, H, W)), (DUMMY + 4, 1, (1, H, W)), (DUMMY + 8, 40, (1, H, W))]


def test_a_good_list_gives_its_total():
    assert lib().ebcc_hip_groups_check(H, W, table(GOOD), len(GOOD)) == 44
    assert lib().ebcc_hip_groups_check(H, W, table(GOOD[:1]), 1) == 3
    # chunk_dims are ignored
    t = table(GOOD)
    t[1].config.chunk_dims[:] = (5, 6, 7)
    assert lib().ebcc_hip_groups_check(H, W, t, len(GOOD)) == 44


def test_every_refusal_has_a_message():
    big = (1 << 63) + 5
    refused = {
        "no groups": (H, W, GOOD, 0),
        "a group without frames": (H, W, GOOD[:1] + [(DUMMY, 0, (1, H, W))], 2),
        "a group with a null pointer": (H, W, GOOD[:2] + [(None, 2, (1, H, W))], 3),
        "dims of several frames": (H, W, GOOD[:1] + [(DUMMY, 2, (2, H, W))], 2),
        "dims of another height": (H, W, [(DUMMY, 2, (1, H + 1, W))], 1),
        "dims of another width": (H, W, GOOD + [(DUMMY, 2, (1, H, W - 1))], 4),
        "a height the engine refuses": (2048, W, [(DUMMY, 2, (1, 2048, W))], 1),
        "a width the engine refuses": (H, 0, [(DUMMY, 2, (1, H, 0))], 1),
        "a total that overflows": (H, W, [(DUMMY, big, (1, H, W)), (DUMMY, big, (1, H, W))], 2),
        "a total whose bytes overflow": (H, W, [(DUMMY, 1 << 60, (1, H, W))], 1),
    }
    for what, (h, w, items, n) in refused.items():
        assert lib().ebcc_hip_groups_check(H, W, table(GOOD), len(GOOD)) == 44          # (a good call in between)
        assert lib().ebcc_hip_groups_check(h, w, table(items), n) == -1, what
        assert error(), what
    assert lib().ebcc_hip_groups_check(H, W, None, 3) == -1 and error()

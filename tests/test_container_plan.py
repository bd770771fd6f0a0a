"""CPU tests of ebcc_hip_container_plan (include/ebcc_hip.h): the chunk dims and the chunk count ebcc_encode_chunking (compat 0) and
ebcc_encode_chunking_compat (compat 1) use for a config, against a restatement of the two rules
(/root/reference/src/ebcc_codec.c:924-964, :1059-1076), and every refusal.  The library loads without a device; a missing symbol
fails."""
import ctypes

import pytest

from tests import _lib as L

SENTINEL = 0xC3C3C3C3
LO, HI = 32, 2047                                                  # EBCC_MIN / MAX_INTERNAL_IMAGE_DIM


def container_plan(dims, chunk_dims, compat):
    """-> ((chunk dims), chunks) or None when the call refuses (then its outputs keep their bytes and a message is set)"""
    fn = getattr(L.product(), "ebcc_hip_container_plan")          # AttributeError where the feature is missing: a failure, not a skip
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(L.CodecConfig), ctypes.c_int, L.c_size_p, L.c_size_p]
    cfg = L.make_config(dims, chunk_dims)
    cd, n = (ctypes.c_size_t * 3)(SENTINEL, SENTINEL, SENTINEL), ctypes.c_size_t(SENTINEL)
    rc = fn(ctypes.byref(cfg), compat, cd, ctypes.byref(n))
    assert rc in (0, 1)
    if rc:
        assert list(cd) == [SENTINEL] * 3 and n.value == SENTINEL, "outputs written by a call that refuses"
        assert L.product().ebcc_hip_last_error(), "a refusal without a message"
        return None
    return tuple(cd), n.value


def model(dims, chunk_dims, compat):
    """the two rules restated; None: refused"""
    cd = list(chunk_dims or (0, 0, 0))
    if not any(cd):
        cd = [1] + [1024 if d > HI else d for d in dims[1:]] if compat else list(dims)
    if cd[0] == 0 or cd[1] == 0 or not (LO <= cd[0] * cd[1] <= HI and LO <= cd[2] <= HI) or 0 in dims:
        return None
    if dims[0] * dims[1] * dims[2] * 4 >= 1 << 64:
        return None
    if cd[0] != 1 and not 32 <= cd[1] <= 1023:                     # (a chunk of several frames is a tiled image: the product's own limit on its tiles)
        return None
    counts = [-(-d // c) for d, c in zip(dims, cd)]
    return tuple(cd), counts[0] * counts[1] * counts[2]


ACCEPTED = [((3, 70, 100), (1, 32, 48)), ((5, 33, 40), (1, 33, 40)), ((2, 40, 50), (1, 64, 64)), ((32, 1801, 3600), (1, 1024, 1024)),
            ((4, 64, 96), (2, 32, 96)),                            # chunks of two frames: the host entry points take them
            ((1, 64, 96), None), ((1, 2047, 2047), None), ((1, 2048, 2047), None), ((7, 1801, 3600), None), ((2, 2100, 1100), None),
            ((2, 2100, 1100), (1, 1024, 1100)), ((3, 32, 32), (1, 32, 32)), ((1, 5000, 31), (1, 2047, 32))]


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("dims,cd", ACCEPTED, ids=str)
def test_plan_is_the_entry_points_rule(dims, cd, compat):
    assert container_plan(dims, cd, compat) == model(dims, cd, compat)


def test_the_cases_of_the_rules():
    assert container_plan((3, 70, 100), (1, 32, 48), 0) == ((1, 32, 48), 27) == container_plan((3, 70, 100), (1, 32, 48), 1)
    assert container_plan((1, 64, 96), None, 0) == ((1, 64, 96), 1)                        # all zero, plain: the array is the chunk
    assert container_plan((2, 32, 96), None, 0) == ((2, 32, 96), 1)
    assert container_plan((7, 1801, 3600), None, 1) == ((1, 1801, 1024), 28)               # compat: 1024 along an axis above 2047 only
    assert container_plan((7, 2047, 2048), None, 1) == ((1, 2047, 1024), 14)
    assert container_plan((2, 2100, 1100), None, 1) == ((1, 1024, 1100), 6)
    assert container_plan((2, 2100, 1100), None, 0) is None                                # 2 x 2100 rows in one chunk
    assert container_plan((2, 2100, 1100), (1, 1024, 1024), 0) == ((1, 1024, 1024), 12)


BIG = 1 << 62
REFUSED = [("chunk rows below 32", (3, 70, 100), (1, 31, 48)), ("chunk columns below 32", (3, 70, 100), (1, 32, 31)),
           ("chunk rows above 2047", (3, 4000, 100), (1, 2048, 48)), ("chunk columns above 2047", (3, 70, 4000), (1, 32, 2048)),
           ("frames x rows above 2047", (4, 1024, 100), (2, 1024, 100)), ("a zero chunk axis", (3, 70, 100), (1, 0, 48)),
           ("a zero leading chunk axis", (3, 70, 100), (0, 32, 48)), ("zero frames", (0, 70, 100), (1, 32, 48)),
           ("zero rows", (3, 0, 100), (1, 32, 48)), ("zero columns", (3, 70, 0), (1, 32, 48)), ("all zero", (0, 0, 0), None),
           ("dims whose product overflows", (BIG, 70, 100), (1, 32, 48)), ("dims whose product overflows", (8, BIG, BIG), (1, 32, 48)),
           ("bytes that overflow", (1 << 40, 1 << 11, 1 << 11), (1, 1024, 1024)),
           ("a chunk of several frames of too few rows", (4, 16, 96), (2, 16, 96))]


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("what,dims,cd", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals(what, dims, cd, compat):
    assert model(dims, cd, compat) is None
    assert container_plan(dims, cd, compat) is None, what

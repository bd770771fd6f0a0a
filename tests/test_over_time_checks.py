"""CPU test of what the five checks of the decodes over time share (ebcc_hip_time_stats_check, ebcc_hip_time_ranks_check,
ebcc_hip_pair_stats_check, ebcc_hip_spell_stats_check, ebcc_hip_time_map_check; include/ebcc_hip.h): for the same bad frame,
window, bin list or count every one of them answers -1 with the same message behind its own name - the noun aside, "frame" for
the reduce, quantile and time-map decodes and "step" for the pair and spell decodes -, and that message is the text these calls
have always given (written out here, not taken from the library).  Where two things are wrong, the frame is named before the
bins.  The time-map decode has no bins: it is in every case that has none.  The library loads without a device; a missing
symbol is an AttributeError - a failure, not a skip."""
import ctypes

import numpy as np
import pytest

from ebcc_amd.h5_batch import PairStats, SpellStats, TimeMap, TimeRanks, TimeStats
from tests import _lib as L

NO_BIN = 0xFFFFFFFF
H, W, N_BINS = 64, 96, 4
COUNT = np.zeros(8, np.uint64)
RANK = np.zeros((N_BINS, 1), np.uint64)
START, FRAME, WEIGHT, FAR_FRAME = np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0]), np.array([7], np.uint32)
SIZE = ctypes.c_size_t


def pointers(spec, names):
    """(the checks never follow a device pointer: any address of the right alignment stands for one)"""
    for k, name in enumerate(names):
        setattr(spec, name, 0x1000 * (k + 1))
    spec.count = COUNT.ctypes.data
    return spec


def time_stats():
    return pointers(TimeStats(N_BINS, H, W, threshold=0.5), ("d_sum", "d_sum_sq", "d_min", "d_max", "d_over"))


def time_ranks():
    return pointers(TimeRanks(N_BINS, H, W, 1, RANK.ctypes.data), ("d_out",))


def pair_stats():
    return pointers(PairStats(N_BINS, H, W, threshold=0.5),
                    ("d_sum_x", "d_sum_y", "d_sum_xx", "d_sum_yy", "d_sum_xy", "d_sum_mag", "d_max_mag", "d_over_mag"))


def spell_stats():
    return pointers(SpellStats(N_BINS, H, W, 0.5, 0, 2), ("d_run", "d_longest", "d_longest_end", "d_spells", "d_spell_steps", "d_events", "d_first",
                                                         "d_last", "d_min", "d_max", "d_when_min", "d_when_max"))


def time_map():
    return pointers(TimeMap(1, H, W, START.ctypes.data, FRAME.ctypes.data, WEIGHT.ctypes.data), ("d_acc",))


# call -> (its spec, its noun, its arguments between the spec and the count: the bins, and the spell decode's labels)
CALLS = {"ebcc_hip_time_stats_check": (time_stats, "frame", 1), "ebcc_hip_time_ranks_check": (time_ranks, "frame", 1),
         "ebcc_hip_pair_stats_check": (pair_stats, "step", 1), "ebcc_hip_spell_stats_check": (spell_stats, "step", 2),
         "ebcc_hip_time_map_check": (time_map, "frame", 0)}
BINNED = [c for c in CALLS if CALLS[c][2]]


def answer(call, height=H, width=W, bins=(0, 1, 1, 0, 2, 3), n=None, row0=0, col0=0, spec=None):
    """what `call` returns and the message it leaves, its own name and ": " taken off"""
    make, _, lists = CALLS[call]
    fn = getattr(L.product(), call)
    fn.restype = ctypes.c_long
    fn.argtypes = [SIZE, SIZE, ctypes.c_void_p] + [ctypes.c_void_p] * lists + [SIZE, SIZE, SIZE]
    spec = make() if spec is None else spec
    b = None if bins is None else np.asarray(bins, np.uint32)
    n = n if n is not None else len(b) if lists else 1
    got = fn(height, width, ctypes.addressof(spec), *([None if b is None else b.ctypes.data, None][:lists]), n, row0, col0)
    text = (L.product().ebcc_hip_last_error() or b"").decode()
    assert got >= 0 or text.startswith(call + ": ")
    return got, text[len(call) + 2:]


@pytest.mark.parametrize("call", list(CALLS))
def test_the_specs_are_accepted(call):
    assert answer(call)[0] == (6 if CALLS[call][2] else 1)


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("bad, text", [
    (dict(height=2048), "unsupported geometry 2048 x 96"),
    (dict(width=0), "unsupported geometry 64 x 0"),
    (dict(row0=1), "the window [1, +64) x [0, +96) is not inside the 64 x 96 frame"),
    (dict(col0=1), "the window [0, +64) x [1, +96) is not inside the 64 x 96 frame"),
    (dict(n=2 ** 63, bins=None), "too many {noun}s"),
])
def test_frame_window_and_count(call, bad, text):
    assert answer(call, **bad) == (-1, text.format(noun=CALLS[call][1]))


@pytest.mark.parametrize("call", BINNED)
@pytest.mark.parametrize("bins, text", [
    ((0, N_BINS, 1), "{noun} 1 names bin 4 of 4"),
    ((NO_BIN, NO_BIN, NO_BIN), "no {noun} is named"),
])
def test_bins(call, bins, text):
    assert answer(call, bins=bins) == (-1, text.format(noun=CALLS[call][1]))


@pytest.mark.parametrize("call", list(CALLS))
def test_the_frame_is_named_before_the_bins(call):
    spec = None
    if call == "ebcc_hip_time_map_check":                              # (no bins: a term that names a frame the call does not have)
        spec = time_map()
        spec.frame = FAR_FRAME.ctypes.data
    assert answer(call, height=2048, bins=(0, N_BINS, 1), spec=spec) == (-1, "unsupported geometry 2048 x 96")
    assert answer(call, bins=(0, N_BINS, 1), spec=spec)[0] == -1

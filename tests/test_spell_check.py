"""CPU tests of ebcc_hip_spell_stats_check (include/ebcc_hip.h): everything the spell decode refuses before it touches a device,
each refusal with a message that names the call and says what is wrong, the neighbour one step inside every limit accepted, the
count it returns and the defaults for a NULL bin and a NULL when.  The library loads without a device (as test_window_plan.py
relies on); a missing symbol is an AttributeError - a failure, not a skip."""
import ctypes

import numpy as np
import pytest

from tests import _lib as L

NO_BIN = 0xFFFFFFFF
NO_STEP = 0xFFFFFFFF
H, W = 64, 96
CALL = "ebcc_hip_spell_stats_check"
RUNS = ("d_run", "d_longest", "d_longest_end", "d_spells", "d_spell_steps")
EVENTS = ("d_events", "d_first", "d_last")
EXTREMES = ("d_min", "d_max", "d_when_min", "d_when_max")
FIELDS = RUNS + EVENTS + EXTREMES


class SpellStats(ctypes.Structure):
    """ebcc_hip_spell_stats"""
    _fields_ = [("n_bins", ctypes.c_size_t), ("rows", ctypes.c_size_t), ("cols", ctypes.c_size_t),
                ("threshold", ctypes.c_float), ("below", ctypes.c_int), ("min_len", ctypes.c_uint32)] + \
               [(name, ctypes.c_void_p) for name in FIELDS] + [("count", ctypes.c_void_p)]


def check_fn():
    fn = L.product().ebcc_hip_spell_stats_check
    fn.restype = ctypes.c_long
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(SpellStats), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                   ctypes.c_size_t]
    return fn


def last_error():
    return (L.product().ebcc_hip_last_error() or b"").decode()


COUNT = np.zeros(8, np.uint64)


def stats(n_bins=4, rows=H, cols=W, count=True, threshold=0.5, below=0, min_len=2, only=None, **ptrs):
    """every array set (the check never follows a device pointer: any address of the right alignment stands for one), or `only`"""
    s = SpellStats(n_bins, rows, cols, threshold, below, min_len)
    for k, name in enumerate(FIELDS):
        setattr(s, name, 0x1000 * (k + 1) if only is None or name in only else None)
    s.count = COUNT.ctypes.data if count else None
    for name, value in ptrs.items():
        setattr(s, name, value)
    return s


def run(s, bins=(0, 1, 1, 0, 2), when=None, height=H, width=W, row0=0, col0=0, n_steps=None):
    b = None if bins is None else np.asarray(bins, np.uint32)
    t = None if when is None else np.asarray(when, np.uint32)
    n = n_steps if n_steps is not None else len(b) if b is not None else len(t)
    return check_fn()(height, width, None if s is None else ctypes.byref(s), None if b is None else b.ctypes.data, None if t is None else t.ctypes.data,
                      n, row0, col0)


def refused(*args, says=(), **kw):
    """-1, with a message that names the call and holds every word of `says`"""
    got = run(*args, **kw)
    text = last_error()
    return got == -1 and CALL in text and len(text) > len(CALL) + 2 and all(word in text for word in says)


def test_struct_layout():
    assert ctypes.sizeof(SpellStats) == 18 * 8 and SpellStats.threshold.offset == 24 and SpellStats.below.offset == 28
    assert SpellStats.min_len.offset == 32 and SpellStats.d_run.offset == 40 and SpellStats.count.offset == 17 * 8


def test_accepts_and_counts_the_named_steps():
    assert run(stats()) == 5
    assert run(stats(), bins=[0, NO_BIN, 3, NO_BIN, NO_BIN, 1]) == 3
    assert run(stats(n_bins=1), bins=[0]) == 1
    assert run(stats(), when=[7, 3, 3, 0, NO_STEP - 1]) == 5                 # (labels need not increase, and may repeat)


def test_defaults_for_a_null_bin_and_a_null_when():
    assert run(stats(), bins=None, n_steps=7) == 7                           # (no bin list: every step in bin 0)
    assert run(stats(n_bins=1), bins=None, when=[5, 6, 7]) == 3
    assert refused(stats(), bins=None, when=[5, NO_STEP, 7], says=("step 1", "label"))
    # (no label list: step f has the label f - a NO_STEP among the labels of others does not matter where the step is skipped)
    assert run(stats(), bins=[0, NO_BIN, 1], when=[1, NO_STEP, 2]) == 2


def test_null_stats_and_null_count():
    assert refused(None)
    assert refused(stats(count=False), says=("count",))


def test_every_device_array_null():
    assert refused(stats(only=()), says=("NULL",))
    for keep in ("d_run", "d_events", "d_first", "d_last", "d_min", "d_max"):    # (one that needs no other is enough)
        assert run(stats(only=(keep,))) == 5, keep


def test_zero_dimensions():
    for name in ("n_bins", "rows", "cols"):
        assert refused(stats(**{name: 0})), name
    assert run(stats(n_bins=3, rows=1, cols=1)) == 5


def test_window_inside_the_frame():
    assert run(stats(rows=40, cols=30), row0=H - 40, col0=W - 30) == 5      # (ends with the frame)
    assert refused(stats(rows=40, cols=30), row0=H - 39, col0=0, says=("window",))
    assert refused(stats(rows=40, cols=30), row0=0, col0=W - 29)
    assert refused(stats(rows=H + 1, cols=W))
    assert refused(stats(rows=H, cols=W + 1))
    assert refused(stats(rows=1, cols=1), row0=H, col0=0)
    assert refused(stats(rows=1, cols=1), row0=0, col0=W)
    assert run(stats(rows=1, cols=1), row0=H - 1, col0=W - 1) == 5
    assert refused(stats(rows=1, cols=1), row0=2 ** 64 - 1, col0=0)         # (row0 + rows wraps)
    assert refused(stats(rows=1, cols=1), row0=0, col0=2 ** 64 - 1)


def test_alignment():
    for name in FIELDS:
        for off in (1, 2, 3):
            assert refused(stats(**{name: 0x3000 + off}), says=("4-byte",)), (name, off)
        assert run(stats(**{name: 0x3004})) == 5, name


def test_runs_arrays_need_d_run():
    for name in RUNS[1:]:
        assert refused(stats(only=(name,) + (("d_longest",) if name == "d_longest_end" else ())), says=("d_run",)), name
        assert refused(stats(only=EVENTS + EXTREMES + (name, "d_longest")), says=("d_run",)), name
    assert run(stats(only=("d_run", "d_spells"))) == 5
    assert run(stats(only=("d_run", "d_spell_steps"))) == 5
    assert run(stats(only=("d_run", "d_longest"))) == 5


def test_longest_end_needs_d_longest():
    assert refused(stats(only=("d_run", "d_longest_end")), says=("d_longest_end", "d_longest"))
    assert run(stats(only=("d_run", "d_longest", "d_longest_end"))) == 5


def test_spells_need_a_min_len():
    assert refused(stats(min_len=0), says=("min_len",))
    assert refused(stats(min_len=0, only=("d_run", "d_spells")), says=("min_len",))
    assert refused(stats(min_len=0, only=("d_run", "d_spell_steps")), says=("min_len",))
    assert run(stats(min_len=0, d_spells=None, d_spell_steps=None)) == 5    # (not looked at without them)
    assert run(stats(min_len=1)) == 5
    assert run(stats(min_len=NO_STEP)) == 5


def test_labels_of_extremes_need_their_extreme():
    assert refused(stats(d_max=None), says=("d_when_max", "d_max"))
    assert refused(stats(d_min=None), says=("d_when_min", "d_min"))
    assert refused(stats(only=("d_when_max", "d_min")), says=("d_when_max",))
    assert refused(stats(only=("d_when_min", "d_max")), says=("d_when_min",))
    assert run(stats(d_max=None, d_when_max=None)) == 5
    assert run(stats(d_min=None, d_when_min=None)) == 5
    assert run(stats(only=("d_max", "d_when_max"))) == 5


def test_threshold():
    nan = float("nan")
    assert refused(stats(threshold=nan), says=("threshold",))
    for name in RUNS[:1] + EVENTS:                                           # (any runs or events array)
        assert refused(stats(threshold=nan, only=EXTREMES + (name,)), says=("threshold",)), name
    assert run(stats(threshold=nan, only=EXTREMES)) == 5                     # (not looked at by the extremes)
    assert run(stats(threshold=float("inf"))) == 5
    assert run(stats(threshold=-1.0, below=1)) == 5


def test_bins():
    assert refused(stats(n_bins=4), bins=[0, 1, 4], says=("bin", "step 2"))
    assert run(stats(n_bins=4), bins=[0, 1, 3]) == 3
    assert refused(stats(n_bins=4), bins=[0, 1, NO_BIN - 1])
    assert refused(stats(), bins=[NO_BIN, NO_BIN], says=("no step",))        # (no step named)
    assert refused(stats(), bins=[], n_steps=0)
    assert run(stats(), bins=[NO_BIN, 2]) == 1


def test_a_named_step_with_the_label_no_step():
    assert refused(stats(), when=[0, 1, NO_STEP, 3, 4], says=("step 2", "label"))
    assert run(stats(), bins=[0, 1, NO_BIN, 0, 2], when=[0, 1, NO_STEP, 3, 4]) == 4      # (the step is skipped: its label is not looked at)
    assert run(stats(), when=[0, 1, NO_STEP - 1, 3, 4]) == 5


@pytest.mark.parametrize("h,w,ok", [(2047, 2047, True), (2048, 96, False), (64, 2048, False), (0, 96, False), (64, 0, False)])
def test_geometry_of_the_frame(h, w, ok):
    s = stats(rows=1, cols=1)
    if ok:
        assert run(s, height=h, width=w) == 5
    else:
        assert refused(s, height=h, width=w, says=("geometry",))

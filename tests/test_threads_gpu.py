"""GPU: concurrent callers get the bytes a serial caller gets.

INTEGRATION.md states what a multi-threaded caller may rely on (entry points serialised per device, engines cached per device
and frame geometry, the last error text per thread, h5_batch's cached codecs shared between threads).  Every test here starts
one fresh child process - `python -m tests._threads <scenario>`, see that module for the shape all scenarios share - whose
threads call the library at once, and asserts on the child's exit status and on its last line.  All comparisons in the child are
exact: `==` on streams, np.array_equal on fields, against the CPU oracle.  ctypes drops the GIL for the length of every call,
so the threads do overlap inside the library.

The time limit of a child, 600 s, is the one the suite's other child-process GPU tests use (tests/test_codec_gpu.py,
tests/test_workspace_gpu.py, ...).  It is a hang guard - a deadlock in the library is a failed test with the child's trail in
the message - not a performance claim.  Measured on an MI355X (one run, this suite's shapes): serial phase (the inputs and the
oracle, after the imports) / threaded phase (engine creation included) / the whole child as pytest times it, in seconds:

    ref_one_geometry       0.30 / 0.35 / 1.20      ref_with_chunk         0.51 / 0.21 / 1.27
    ref_four_geometries    0.16 / 0.22 / 0.95      zarr_pool              0.93 / 0.40 / 1.98
    context_families       2.16 / 0.23 / 2.84      shared_context         0.65 / 0.08 / 1.24
    unlocked_helpers       0.16 / 0.16 / 0.77      release_beside_calls   0.26 / 0.23 / 0.97
    last_error_per_thread  0.05 / 0.05 / 0.65      (create_keeps_device: that box has one device)

No scenario widens a window with a sleep or repeats itself to catch a rare interleaving, and none is run against a build
without the device lock: the lock scenarios are argued in their docstrings (which object the threads share), the last-error
scenario was shown red once on a host-only mutation (the error text not thread_local)."""
import os
import subprocess
import sys

import pytest

from tests import _hard_bound as HB
from tests import _lib as L

pytestmark = pytest.mark.gpu

LIMIT = 600                                           # seconds: what the suite's other child processes get


def child(scenario):
    """run one scenario in a fresh process -> its stdout lines; fails with the child's trail unless it ended with `compared`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("EBCC_HIP_") and k not in HB.ENV_NAMES}
    try:
        r = subprocess.run([sys.executable, "-m", "tests._threads", scenario], capture_output=True, text=True, env=env, cwd=L.ROOT, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"{scenario}: no end within {LIMIT} s - a deadlock?  The child's trail:\n{out}")
    lines = r.stdout.strip().splitlines()
    print("\n".join(lines))
    assert r.returncode == 0 and lines and lines[-1] == "compared", (scenario, r.returncode, lines, r.stderr[-2000:])
    return lines


def test_reference_api_four_threads_one_geometry():
    """Scenario 1.  Four threads call ebcc_encode and ebcc_decode on their own 64 x 96 frames - MAX_ERROR, RELATIVE_ERROR, NONE
    and constant fields.  What they share is the ONE cached engine of (device 0, 64 x 96): its d_io buffer, into which every
    call uploads its frame and from which every decode is downloaded, and its workspace (coefficients, bit-plane lists, the
    search's state).  Without the device lock two calls would upload into, search over and read back the same buffers at once:
    a thread would get the stream or the field of another thread's frame, or a mixture."""
    lines = child("ref_one_geometry")
    assert sum(1 for l in lines if l.startswith("thread ")) == 4


def test_reference_api_with_a_multi_frame_chunk():
    """Scenario 1 with the frames of thread 0 being one (4, 96, 160) chunk: the tiled path, whose call takes two engines
    (chunk_engines: the tiles' and the stacked image's) from the map while the other threads use and the map holds theirs."""
    child("ref_with_chunk")


def test_reference_api_four_geometries():
    """Scenario 2.  33 x 47, 64 x 96, 96 x 160 and 100 x 130 at once, then every thread moves to the next geometry: the engine
    map grows from empty under four threads, and every engine is made by one thread and used next by another."""
    child("ref_four_geometries")


def test_zarr_codec_on_a_thread_pool():
    """Scenario 3.  Sixteen chunks of two geometries through EBCCZarrFilter.encode, .decode and .decode(out=) on a
    concurrent.futures.ThreadPoolExecutor(4), as Zarr drives a codec."""
    child("zarr_pool")


def test_one_context_per_thread_four_families_of_calls():
    """Scenario 4.  Four threads, each with contexts of eight 64 x 96 frames of its own, each a family of calls: encode_frames /
    decode_frames; encode_shard of twelve frames (more than the context holds: its second engine set is made while the others
    run - twelve, not the eight frames a call has elsewhere in this file, because the context is to hold eight); the audit and
    the hard-bound encode; window and box decode, reduce and series.  Expected bytes and helpers are those of the families' own
    single-thread tests."""
    child("context_families")


def test_one_context_shared_by_two_threads():
    """Scenario 5.  Both threads call ebcc_hip_encode_frames and ebcc_hip_decode_frames on the ONE ctx, each with device buffers
    of its own.  The context's whole workspace, its streams and its pinned tables are one set; only the per-device lock keeps
    one thread's batch from being coded into the other's.  Without it the streams of the two batches would mix."""
    child("shared_context")


def test_unlocked_helpers_beside_a_running_call():
    """Scenario 6.  ebcc_hip_create / _destroy of another geometry and ebcc_hip_malloc / _memcpy_h2d / _memcpy_d2h / _free - none
    of which takes the device lock - beside a thread that encodes: the encoder's streams and the copied buffer are intact."""
    child("unlocked_helpers")


def test_release_engines_beside_calls():
    """Scenario 7.  Two workers make six one-frame calls each while a third thread calls ebcc_hip_release_engines three times,
    once after each barrier the workers pass: every call succeeds (a released engine is made again) with the oracle's bytes."""
    child("release_beside_calls")


def test_last_error_is_per_thread():
    """Scenario 8.  Thread A's ebcc_hip_prepare(ctx, max_frames + 1) is refused on the host ("bad batch") while thread B
    encodes successfully; afterwards A reads its own text and B does not see it."""
    child("last_error_per_thread")


def test_create_keeps_the_callers_device():
    """Scenario 9.  With device 0 current (torch.cuda.set_device), ebcc_hip_create(1, ...) and ebcc_hip_destroy leave it current."""
    if L.product().ebcc_hip_device_count() < 2:
        pytest.skip("needs two devices")
    child("create_keeps_device")

"""CPU: the codec cache of ebcc_amd/h5_batch.py under two threads, with a fake BatchCodec - no device, no library call.

The fake records `create`, `close`, and `enter` / `leave` of its encode in one list under a lock, and its encode blocks on an
Event the test sets: the order of the records is the order of the events, so "closed while a call was inside" is a plain fact
of the list.  No case sleeps: a thread that must have come to rest before the next step is waited for through an Event of its
own, and every join has a time limit whose expiry is a failure (a deadlock in the cache is a red test, not a stuck suite).

A user of a cached codec goes through h5_batch.write_frames itself, on a fake dataset that keeps the chunks it is handed."""
import threading

import numpy as np
import pytest

from ebcc_amd import h5_batch

H, W = 64, 96
JOIN = 30.0                                           # seconds; nothing here takes a measurable time unless it deadlocks


class Log:
    def __init__(self):
        self.lock, self.events = threading.Lock(), []

    def add(self, what, codec):
        with self.lock:
            self.events.append((what, codec.serial))

    def of(self, serial):
        with self.lock:
            return [what for what, s in self.events if s == serial]

    def count(self, what):
        with self.lock:
            return sum(1 for w, _ in self.events if w == what)


def fake_codec_class(log, entered, go):
    """a BatchCodec that has no engine: encode sets `entered`, waits for `go` and gives one stream per frame"""
    serials = iter(range(1, 1000))

    class FakeCodec:
        def __init__(self, height, width, max_frames=256, device=0):
            self.h, self.w, self.max_frames, self.ctx = int(height), int(width), int(max_frames), object()
            self.serial = next(serials)
            log.add("create", self)

        def close(self):
            if self.ctx:
                log.add("close", self)
                self.ctx = None

        def encode(self, frames, cfg, hard=False, max_rounds=0):
            log.add("enter", self)
            alive = self.ctx is not None
            entered.set()
            assert go.wait(JOIN), "the test never let the encode go on"
            alive = alive and self.ctx is not None                 # (an engine destroyed under the call)
            log.add("leave" if alive else "leave without an engine", self)
            return [b"stream %d" % i for i in range(len(frames))]

    return FakeCodec


class FakeDataset:
    """what write_frames asks of an h5py dataset of one-frame chunks"""
    name = "/fake"

    def __init__(self, n):
        self.shape, self.chunks, self.written = (n, H, W), (1, H, W), {}
        self.id = self

    def write_direct_chunk(self, offset, data, filter_mask=0):
        self.written[offset] = data


@pytest.fixture
def cache(monkeypatch):
    log, entered, go = Log(), threading.Event(), threading.Event()
    monkeypatch.setattr(h5_batch, "BatchCodec", fake_codec_class(log, entered, go))
    h5_batch.close_cached()                           # (nothing of another test's)
    yield log, entered, go
    go.set()
    h5_batch.close_cached()


def run(fn):
    """fn on a thread of its own -> (thread, box): box holds the result or the exception"""
    box = []

    def body():
        try:
            box.append(fn())
        except BaseException as e:                    # noqa: B902 (handed to the test's thread)
            box.append(e)

    t = threading.Thread(target=body, daemon=True)
    t.start()
    return t, box


def finish(*threads):
    for t, box in threads:
        t.join(JOIN)
        assert not t.is_alive(), "a thread did not finish: the cache deadlocked"
        assert box and not isinstance(box[0], BaseException), box


def writer(n_frames):
    dset = FakeDataset(n_frames)
    data = np.zeros((n_frames, H, W), np.float32)
    return dset, lambda: h5_batch.write_frames(dset, data, 10.0)


def closed_inside(log, serial):
    """was codec `serial` closed between an enter and the leave that follows it?"""
    inside = False
    for what in log.of(serial):
        if what == "enter":
            inside = True
        elif what.startswith("leave"):
            inside = False
        elif what == "close" and inside:
            return True
    return False


def test_a_larger_request_waits_for_the_user_of_the_cached_codec(cache):
    """Thread A is inside encode on the cached codec for (64, 96) of 4 frames when thread B asks for 8: B must not close A's
    codec under it, B ends with a codec of at least 8 frames, and both finish."""
    log, entered, go = cache
    dset, write = writer(4)
    a = run(write)
    assert entered.wait(JOIN)                          # A is inside encode of codec 1 (max_frames 4)
    b = run(lambda: h5_batch.cached_codec(H, W, 8))
    # B is now waiting for A or - the fault - closing codec 1.  Neither can be waited for without a time limit running out,
    # and need not be: a request that never waits is microseconds of Python that keep the interpreter until they are done
    # (a started thread runs until it blocks), so a cache that closes under its user has done so before A is let go here;
    # the records are in the order things happened.
    go.set()
    finish(a, b)
    assert log.of(1)[:2] == ["create", "enter"], log.events
    assert not closed_inside(log, 1), log.events
    assert "leave" in log.of(1) and "leave without an engine" not in log.of(1), log.events
    got = b[1][0]
    assert got.max_frames >= 8 and got.ctx, log.events
    assert h5_batch.cached_codec(H, W, 8) is got
    assert log.of(1)[-1] == "close" and log.count("create") == 2, log.events       # (replaced once A had left)
    assert len(dset.written) == 4


def test_close_cached_waits_for_the_user(cache):
    log, entered, go = cache
    dset, write = writer(3)
    a = run(write)
    assert entered.wait(JOIN)
    b = run(h5_batch.close_cached)
    go.set()
    finish(a, b)
    assert not closed_inside(log, 1), log.events
    assert log.of(1) == ["create", "enter", "leave", "close"], log.events
    assert len(dset.written) == 3
    assert h5_batch.cached_codec(H, W, 3).serial == 2          # (the cache was emptied: the next request makes a codec)


def test_two_requests_for_a_missing_geometry_make_one_codec(cache):
    log, _entered, _go = cache
    gate = threading.Barrier(2)

    def ask():
        gate.wait(JOIN)
        return h5_batch.cached_codec(H, W, 4)

    a, b = run(ask), run(ask)
    finish(a, b)
    assert a[1][0] is b[1][0] and log.count("create") == 1, log.events


def test_held_codec_hands_a_callers_own_codec_through(cache):
    log, _entered, _go = cache
    own = h5_batch.BatchCodec(H, W, 2)
    with h5_batch.held_codec(H, W, 2, codec=own) as c:
        assert c is own and not h5_batch._holders
    assert not h5_batch._codecs and log.of(own.serial) == ["create"]      # (not cached, not closed)
    with h5_batch.held_codec(H, W, 2) as c:
        assert c is not own and h5_batch._holders == {c: 1}
        with h5_batch.held_codec(H, W, 1) as again:                          # (a smaller request inside: the same codec, held twice)
            assert again is c and h5_batch._holders == {c: 2}
    assert not h5_batch._holders and h5_batch.cached_codec(H, W, 2) is c

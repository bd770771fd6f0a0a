"""The catalogue of tests/test_spiht_cuts.py (CPU) and tests/test_spiht_cuts_gpu.py: the residual coder at every bit budget
and every cut of its stream.

k_spiht_decode cuts the next 64 stream bits into list entries with closed forms and applies the reference's
`if (++bit_cnt > bits) return;` tests (src/spiht/spiht_re.c:334-426) afterwards, per lane; k_spiht_encode trims an entry to the
bits left; k_reconstruct rebuilds the decoder's state from bookkeeping.  What those do at the budget depends on the kind of bit
the budget falls on (a significance bit whose sign is the next bit, a set bit, a child's bit, a refinement bit, a type-B entry,
the last lane of a chunk), so the cuts here are bit-granular.

Geometries: (32, 32) - 16 LL entries, the seed loop's single partial chunk; (33, 47) - crop both ways; (64, 130) - 144 LL
entries, the seed loop runs three times; (40, 2047) - 1536 LL entries, passes many chunks long.
Images: full-range noise, the checkerboard, a single spike, a smooth field, and a field whose sets are all significant on one
bit-plane (9-bit list entries).
The stream of a case is the oracle's at STREAM_BITS; at 32 x 32 the coder runs out of bit-planes before that budget, and those
streams end through the last bit-plane, not through the budget.

No GPU import here."""
import functools
import hashlib
import struct

import numpy as np

from tests import _fields as F
from tests import _lib as L

GEOMS = [(32, 32), (33, 47), (64, 130), (40, 2047)]
SMALL = GEOMS[:2]
IMAGES = ["noise", "checker", "spike", "smooth", "dense"]
CASES = [(h, w, name) for (h, w) in GEOMS for name in IMAGES]
STREAM_BITS = 8 * 1600
BITS0 = STREAM_BITS + 128                                                # the header's bits0 (spiht_re.c:458)
WINDOW = 512                                                             # cuts, or budgets, per digest of the fixture
PER_CALL = 64                                                            # frames per call of the GPU tests


def case_id(case):
    return "{}x{}-{}".format(*case)


def dense(h, w):
    """the third image of tests/test_residual_gpu.py::test_dense_planes_bit_exact at any size"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (0.5 + 0.5 * ((xx % 2) * 2 - 1) * ((yy % 2) * 2 - 1) * (0.25 + 0.75 * ((xx * 7 + yy * 13) % 5) / 4)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def image(h, w, name):
    if name == "noise":
        a = F.field("noise", h, w, 7)
    elif name == "smooth":
        a = L.smooth_image(h, w, 3)
    elif name == "dense":
        a = dense(h, w)
    else:
        a = F.field(name, h, w)
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def stream(h, w, name):
    """the oracle's stream of the case at STREAM_BITS"""
    return L.orc_spiht_encode(image(h, w, name), STREAM_BITS)


@functools.lru_cache(maxsize=None)
def unbudgeted_bits(h, w, name):
    """length in bits of the oracle's stream with no budget (trunc_bits 0), header and padding included"""
    return 8 * len(L.orc_spiht_encode(image(h, w, name), 0))


def decode_cuts(h, w, n):
    """num_bits of the decodes of a stream of n bytes, ascending"""
    end = 8 * n + 40
    if (h, w) in SMALL:
        cuts = set(range(129, end + 1))
    else:
        cuts = set(range(129, 129 + 2048)) | set(range(end - 512, end + 1)) | set(range(136, end + 1, 8))
    cuts = {c for c in cuts if c >= 129}
    cuts |= {BITS0, BITS0 + 1, 2 ** 40}                                  # the clamp to bits0, spiht_re.c:495-499
    return sorted(cuts)


def decode_pairs(h, w, n):
    """(num_bits, size) in catalogue order: each cut with the bytes it needs (the production form: bits past the end read as
    0), then with the whole stream (the bits past the budget are real)"""
    out = []
    for c in decode_cuts(h, w, n):
        out += [(c, min(n, (c + 7) // 8)), (c, n)]
    return out


def encode_budgets(h, w, name):
    """trunc_bits of the encodes, ascending"""
    dense_to = 4096 if (h, w) in SMALL else 1024
    b = {0} | set(range(24, dense_to + 1)) | set(range(1024, 12801, 97)) | {unbudgeted_bits(h, w, name) + 64}
    return sorted(b)


def prefix_cuts(n):
    """bits of the prefixes of ebcc_hip_spiht_decode_prefix: spiht_decode(buf, bits / 8, ..., bits), so byte cuts only"""
    return list(range(136, 8 * n + 1, 8))


def windows(items):
    return [items[i:i + WINDOW] for i in range(0, len(items), WINDOW)]


def interleaved(items, per_call=PER_CALL):
    """items in calls of at most per_call: call k takes every ncalls-th item from the k-th on, so each call spans the whole
    range, and every other call runs backwards, so a slot that held a long stream next holds a short one"""
    ncalls = -(-len(items) // per_call)
    calls = [items[k::ncalls] for k in range(ncalls)]
    return [c[::-1] if k & 1 else c for k, c in enumerate(calls)]


def interleaved_pairs(h, w, n):
    """decode_pairs in calls of at most PER_CALL frames: the cuts interleaved as above, each followed by its second size form,
    the two forms in alternating order"""
    calls = []
    for cuts in interleaved(decode_cuts(h, w, n), PER_CALL // 2):
        call = []
        for i, c in enumerate(cuts):
            forms = [(c, min(n, (c + 7) // 8)), (c, n)]
            call += forms[::-1] if i & 1 else forms
        calls.append(call)
    return calls


MIXED_CALLS = 40                                                         # calls of test_decoder_batches_mix_images per geometry


def mixed_calls(h, w):
    """MIXED_CALLS calls of PER_CALL frames: frame i is image i % 5 at a pair (num_bits, size) scattered over that image's
    decode_pairs by a multiplicative hash; (image name, num_bits, size) per frame"""
    pairs = {name: decode_pairs(h, w, len(stream(h, w, name))) for name in IMAGES}
    per_image = -(-PER_CALL // len(IMAGES))
    calls = []
    for k in range(MIXED_CALLS):
        call = []
        for i in range(PER_CALL):
            name = IMAGES[i % len(IMAGES)]
            q = k * per_image + i // len(IMAGES)
            call.append((name,) + pairs[name][(q * 2654435761 + 12345) % len(pairs[name])])
        calls.append(call)
    return calls


def threaded(fn, jobs, threads=8, batch=64):
    """[fn(*job) for job in jobs], in order, lazily, on a few threads: the oracle keeps no state between calls and ctypes
    releases the interpreter lock for the length of one, and at 40 x 2047 a decode is 2 ms of inverse wavelet"""
    from concurrent.futures import ThreadPoolExecutor
    jobs = list(jobs)
    with ThreadPoolExecutor(threads) as pool:
        for i in range(0, len(jobs), batch):
            yield from pool.map(lambda j: fn(*j), jobs[i:i + batch])


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def digests(case, encode, decode, mapped=lambda fn, jobs: (fn(*j) for j in jobs)):
    """the record of a case in tests/golden/spiht_cuts.json from encode(image, trunc_bits) and decode(stream, h, w, num_bits):
    the reference build's in oracle/make_golden_spiht_cuts.py, the oracle's in tests/test_spiht_cuts.py (mapped: how the calls
    of a window are made, in order)"""
    h, w, name = case
    img = np.array(image(h, w, name))
    s = encode(img, STREAM_BITS)
    rec = {"field_sha256": sha(img.tobytes()), "n": len(s), "stream_sha256": sha(s), "decode": [], "encode": []}
    for win in windows(decode_pairs(h, w, len(s))):
        d = hashlib.sha256()
        for out in mapped(decode, [(s[:size], h, w, num_bits) for num_bits, size in win]):
            d.update(out.tobytes())
        rec["decode"].append(d.hexdigest())
    for win in windows(encode_budgets(h, w, name)):
        d = hashlib.sha256()
        for e in mapped(encode, [(img, tb) for tb in win]):
            d.update(struct.pack("<Q", len(e)) + e)
        rec["encode"].append(d.hexdigest())
    return rec


def totals(h, w):
    """(decodes, budgets, prefix cuts) of a geometry over its images"""
    d = b = p = 0
    for name in IMAGES:
        n = len(stream(h, w, name))
        d += len(decode_pairs(h, w, n))
        b += len(encode_budgets(h, w, name))
        p += len(prefix_cuts(n))
    return d, b, p

"""N>1 path on CPU for a bound that is relative to the GLOBAL range: two gloo ranks shard a frame stack under a RELATIVE_ERROR
config with relative_to_global_range=True (ebcc_amd/sharding.py).  Each rank takes the range of its own block, the ranges are
combined with all_reduce, and every rank codes with the config ebcc_encode_chunking_compat would code with.  The result must be
byte-identical to the oracle's restatement of ebcc_encode_chunking_compat for the whole stack, and differ from the flag-off
result (every frame bounded by its own range).  The per-frame encoder is the CPU oracle standing in for the GPU, as in
test_sharding_gloo.py.  A NaN on one rank makes every rank raise, and no rank is left waiting in a collective."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def stack(n_frames):
    """frame i lifted by 3 i: the global range is no single frame's range"""
    from tests import _lib as L
    return np.stack([L.era5_like(32, 40, 100 + i) + np.float32(3.0 * i) for i in range(n_frames)]).astype(np.float32)


def _worker(rank, world, port, n_frames, nan_at, q):
    import torch.distributed as dist
    from ebcc_amd import sharding
    from tests import _lib as L
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    frames = stack(n_frames)
    if nan_at is not None:
        frames[nan_at] = np.nan
    cfg = L.make_config((1, 32, 40), base_cr=10.0, error=0.01, residual_type=L.RELATIVE_ERROR)
    L.oracle().orc_set_j2k_backend(0)

    def encode_fn(block, config):
        return [L.orc_encode(f, config) for f in block]

    try:
        on = sharding.encode_stack_sharded(frames, cfg, encode_fn, relative_to_global_range=True)
        off = sharding.encode_stack_sharded(frames, cfg, encode_fn)
        assert cfg.residual_compression_type == L.RELATIVE_ERROR and cfg.error == np.float32(0.01)      # the caller's config is not touched
        q.put((rank, "ok", on, off))
    except ValueError as e:
        q.put((rank, "raised", str(e), None))
    dist.barrier()
    dist.destroy_process_group()


def _run(n_frames, nan_at=None):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_frames, nan_at, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r[0], r[1:]) for r in (q.get(timeout=120), q.get(timeout=120)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


@pytest.mark.parametrize("n_frames", [5, 2, 1])
def test_two_ranks_with_the_global_range_equal_the_compat_container(n_frames):
    from tests import _lib as L
    got = _run(n_frames)
    assert got[0][0] == "ok" and got[1][0] == "ok"
    assert got[1][1] is None and got[1][2] is None                                        # the container is rank 0's
    frames = stack(n_frames)
    cfg = L.make_config((n_frames, 32, 40), (1, 32, 40), base_cr=10.0, error=0.01, residual_type=L.RELATIVE_ERROR)
    L.oracle().orc_set_j2k_backend(0)
    assert got[0][1] == L.orc_encode(frames, cfg, "orc_ebcc_encode_chunking_compat")
    plain = L.orc_encode(frames, cfg, "orc_ebcc_encode_chunking")
    assert got[0][2] == plain                                                              # flag off: today's path
    # 5 frames: the global range is wider than any frame's and the two containers differ.  With 2 frames and with 1 the
    # oracle's own compat and plain containers are the same bytes (the wider bound changes no frame's stream there), so
    # there is no difference to ask for.
    assert (got[0][1] != plain) == (n_frames == 5)


def test_a_nan_on_one_rank_raises_on_both():
    got = _run(5, nan_at=(4, 7, 9))                                                        # frames 3, 4 are rank 1's block
    assert got[0][0] == "raised" and got[1][0] == "raised", got
    assert "NaN" in got[0][1] and "NaN" in got[1][1]

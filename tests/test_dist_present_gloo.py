"""Multi-process (world_size 2, gloo, CPU) coverage of FrameGatherer.gather_display (idkengine_amd/dist.py): the ranks' uint8 display rows — what idkptPresent produced for
each rank's rows — are all-gathered with the padding and placement of gather().  The per-rank renderer is synthetic here (no GPU in this container): every rank holds the
rows of one known uint8 image that the deal gives it; on the GPU box GpuShardRenderer.local_display() aliases the library's display buffer instead."""
import os
import sys
import socket
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 70, 47   # odd height: the ranks hold different row counts (24 / 23), so the shorter shard is padded for the collective


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def full_display():
    """(H, W, 4) uint8: every byte depends on its row, column and channel; alpha 255."""
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(4), indexing="ij")
    img = ((y * 37 + x * 11 + c * 101 + (y * x) % 7) % 256).astype(np.uint8)
    img[..., 3] = 255
    return img


class SyntheticDisplayRenderer:
    def __init__(self, rows, row_band=1, exact=False):
        self.row_band, self.exact = row_band, exact
        self._rows = rows
        self.rows, self.width = len(rows), W

    def local_display(self, settings=None, image=0):
        return torch.from_numpy(np.ascontiguousarray(full_display()[self._rows]))


def _worker(rank, world, port, q, layout):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from idkengine_amd import dist as D
    if layout == "strips":
        first, count = D.strip_of_rank(H, world, rank)
        r = SyntheticDisplayRenderer(list(range(first, first + count)), exact=True)
    else:
        r = SyntheticDisplayRenderer(D.rows_of_rank(H, world, rank, layout), row_band=layout)
    frame = D.FrameGatherer(r, W, H)
    assert D.FrameGatherer is D.ShardedFrame
    full = frame.gather_display()
    q.put((rank, full.numpy().copy(), r.rows))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("layout", [1, 8, "strips"])
def test_gather_display_world2_gloo(layout):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, layout)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(60); assert p.exitcode == 0
    want = full_display()
    assert (res[0][2], res[1][2]) == (24, 23)
    for _, full, _ in res:                                             # every rank holds the full display, byte for byte
        assert full.dtype == np.uint8 and full.shape == (H, W, 4) and full.tobytes() == want.tobytes()

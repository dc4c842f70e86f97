"""LossMeter.all_reduce at world size 2 over gloo, on the CPU-emulated kernels: each rank meters half of 10 images; afterwards both
ranks hold, bit for bit, the state of one meter over all 10 (the process harness is that of tests/test_dist_cpu.py)."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, B, PER_SAMPLE = 1000, 10, 3072
TIMESTEPS = [0, 999, 99, 100, 500, 501, 640, 37, 37, 905]


def _worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from bbdm_amd import LossMeter, dist_utils as du
    from emu_backend import emulated_backend
    import loss_meter_cases as C
    dist = du.init(backend="gloo")
    with emulated_backend():
        a, b = C.pair(10, PER_SAMPLE)
        t = torch.tensor(TIMESTEPS, dtype=torch.int64)
        sl = slice(rank * 5, (rank + 1) * 5)
        meter = LossMeter(T, B, device="cpu")
        meter.add(a[sl], b[sl], t[sl])
        own = meter.meter.clone()
        meter.all_reduce()
        q.put((rank, own.tolist(), meter.meter.tolist(), meter.counts.tolist()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_all_reduce_equals_one_meter_over_all_images():
    sys.path[:0] = [os.path.join(ROOT, "tests")]
    world, port = 2, 29631
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=150) for _ in range(world)], key=lambda r: r[0])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    from bbdm_amd import LossMeter
    from emu_backend import emulated_backend
    import loss_meter_cases as C
    with emulated_backend():
        a, b = C.pair(10, PER_SAMPLE)
        whole = LossMeter(T, B, device="cpu")
        whole.add(a, b, torch.tensor(TIMESTEPS, dtype=torch.int64))
    (_, own0, meter0, counts0), (_, own1, meter1, counts1) = res
    assert own0 != own1 and own0 != whole.meter.tolist()
    for meter, counts in ((meter0, counts0), (meter1, counts1)):
        assert torch.equal(torch.tensor(meter, dtype=torch.int64), whole.meter)
        assert torch.equal(torch.tensor(counts, dtype=torch.int64), whole.counts)
    assert int(whole.counts.sum()) == 10

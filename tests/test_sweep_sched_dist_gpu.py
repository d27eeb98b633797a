"""Row shards under the phased sweep schedule (hh_tune "sweep_sched" 2): the
two-processes-on-one-GPU arrangement of tests/test_dist_gpu.py (gloo
exchange, both ranks on cuda:0), with the schedule forced in each child.  A
shard's band sweep then starts behind its flat kernel on the side stream, with
the symmetric band kernels (the Python driver) and with the upper-band sweep
and its halo rows (the C++ loop).  Every rank's weights equal the one-process
run bitwise."""
import os
import socket
import tempfile

import numpy as np
import pytest

from hichap_master_amd import synth
from tests.knobs import tuned

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, case, outdir, impl, uband):
    import torch
    import torch.distributed as tdist
    from hichap_master_amd import _lib, dist, ice
    torch.cuda.set_device(0)
    _lib.load()
    _lib.call("hh_set_device", 0)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # for the life of this child process (the single launch is checked first: off)
        with tuned(conc_min_bytes=0, sweep_single=0, sweep_sched=2, uband=uband):
            b1, b2, c, off = case
            n = int(off[-1])
            rr = dist.partition_rows(np.bincount(b1, minlength=n) + np.bincount(b2, minlength=n), world)
            opts = ice.IceOptions(max_iters=400)
            m = ice.ContactMatrix.from_pixels(b1, b2, c, n, off, row_range=(rr[rank], rr[rank + 1]))
            st = ice.IceState(m, opts)
            sched = st.sweep_sched()
            if impl == "capi":
                st.close()
                cx = dist.CapiExchange(rr, world, rank, backend="gloo")
                w, s_ = dist.balance_capi(m, opts, cx, torch.cuda.current_stream().cuda_stream)
                cx.close()
            else:
                ex = dist.Exchange(rr, torch.device("cuda", 0))
                w, s_ = dist.balance_sharded(st, ex, max_iters=400)
                st.close()
            torch.cuda.synchronize()
            m.close()
        np.save(os.path.join(outdir, f"w{rank}.npy"), w)
        np.save(os.path.join(outdir, f"it{rank}.npy"), np.array([int(s_["iters"]), sched]))
    finally:
        tdist.destroy_process_group()


@pytest.mark.parametrize("impl,uband", [("python", 1), ("capi", 2)])
def test_phased_shards_two_processes(impl, uband):
    import torch.multiprocessing as mp
    from hichap_master_amd import _lib, ice
    _lib.require_gpu()
    rng = np.random.default_rng(21)
    case = synth.coo_genome([900, 700, 400], rng, A=25.0, trans_density=0.01)
    b1, b2, c, off = case
    n = int(off[-1])
    with tuned(uband=uband):  # (the band kernels the shards run; the schedule is the default's)
        w_full, st_full = ice.balance(b1, b2, c, n, off, max_iters=400)
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_worker, args=(2, _free_port(), case, d, impl, uband), nprocs=2, start_method="spawn")
        ws = [np.load(os.path.join(d, f"w{r}.npy")) for r in range(2)]
        its = [np.load(os.path.join(d, f"it{r}.npy")) for r in range(2)]
    for w, it in zip(ws, its):
        np.testing.assert_array_equal(w, w_full)
        assert it.tolist() == [st_full["iters"], 2]  # the one-process iteration count; the phased schedule ran

"""rb_engine_set_timing over the device forms of all four passes: classify, locate, hits and spans bracket their kernels through one
shared helper, and each device-form call leaves exactly one record.  No assertion on how long anything took."""
import numpy as np
import pytest

from readbouncer_amd import capi
from tests import helpers as H


@pytest.mark.gpu
def test_every_device_form_call_leaves_one_timing_record():
    import torch

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    f = capi.DeviceIBF.create(0, 100, 3, 13, 128 * 4096)  # 100 bins: two word columns
    f.fill_synth(3)
    eng = capi.Engine(0, [f], [])
    buf, offs, lens = H.pack_reads([H.random_dna(rng, 100) for _ in range(8)])
    n = len(lens)
    t_seq, t_off, t_len = (torch.from_numpy(a).to(dev) for a in (buf, offs.view(np.int64), lens.view(np.int32)))
    t_q = torch.zeros((n, 2), dtype=torch.int32, device=dev)  # (item, bin) = (0, 0), n times
    t_mc = torch.zeros((n, 1), dtype=torch.int16, device=dev)
    t_u32 = torch.zeros((n, 1), dtype=torch.int32, device=dev)
    t_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    src = (t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, 100)

    eng.set_timing(True)
    eng.classify_device_ex(*src, d_maxcount=t_mc.data_ptr())
    eng.locate_device(*src, d_hit_bins=t_u32.data_ptr())
    eng.hits_device(*src, d_n_hits=t_u32.data_ptr())
    eng.spans_device(*src, 0, t_q.data_ptr(), n, d_status=t_st.data_ptr())
    ms, calls = eng.kernel_time()
    assert calls == 4 and ms > 0.0, (ms, calls)
    ms, calls = eng.kernel_time()  # collected: the ring starts over
    assert calls == 0 and ms == 0.0, (ms, calls)
    eng.destroy()

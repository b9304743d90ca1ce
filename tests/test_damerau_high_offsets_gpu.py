"""strsim_damerau_device / strsim_damerau_distance_device with their columns placed high in the first 4 GiB behind the values
pointer (tests/high_offsets.py), the way tests/test_high_offsets_gpu.py treats strsim_distance_device: one column straddles byte
2^31 inside a short row, the other ends at offset 2^32 - 1.  The results must equal those of the same call at base 0 and the
reference, and so must the tier counter: a byte leaked from outside a column changes a distance or sends a row to the wave tier."""
import random

import numpy as np
import pytest

import damerau_ref as R
import gen
import high_offsets as H

pytestmark = pytest.mark.gpu


def frame():
    rng = random.Random(12)
    A, B = R.lane_frame(rng, 600, 32)
    A2, B2 = gen.pairs(13, 120, gen.MIXED, 0, 80)
    a = gen.rand_string(rng, R.LOWER, 150, 150)  # (a sign_long row)
    return A + A2 + [a, ""], B + B2 + [R.gapped(rng, a, 3, R.LOWER), ""]


def test_dl_device_at_high_offsets():
    import strsim_amd as S
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < H.MIN_FREE:
        pytest.skip("less than 8 GiB of device memory free")
    A, B = frame()
    cref = R.CRef()
    d, s = cref.distances(A, B), cref.scores(A, B)
    hb = H.HighBuffer(torch, "cuda:0")
    torch.cuda.synchronize()
    try:
        with S.Context(0) as ctx:
            counters = {}
            for pa, pb in (("low", "low"), ("sign_short", "top1"), ("top1", "sign_long")):
                hb.reset()
                cols = hb.place_named(A, pa) + hb.place_named(B, pb)
                out = ctx.damerau_device(*cols)
                ctx.synchronize()
                assert np.array_equal(out.cpu().numpy().view(np.uint64), s.view(np.uint64)), (pa, pb)
                counters[(pa, pb, "sim")] = ctx.last_wave_rows
                for k in (None, 2):
                    out = ctx.damerau_distance_device(*cols, k)
                    ctx.synchronize()
                    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.clamp(d, k)), (pa, pb, k)
                    counters[(pa, pb, k)] = ctx.last_wave_rows
            assert len(set(counters.values())) == 1 and 0 < counters[("low", "low", "sim")] < len(A), counters
    finally:
        hb.close()

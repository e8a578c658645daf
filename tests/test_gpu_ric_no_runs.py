"""GPU: `nyx_hip_traj_ric_diff` of NO run (n = 0).  Unlike the other two fused reports the RIC entry goes through its launch
bracket for an empty ensemble - every sample has count 0, so the moments that were asked for come back as zeros - and it is the
one path on which that bracket runs without a kernel."""
import ctypes as C

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi
from scenarios import leo_full_setup

pytestmark = pytest.mark.gpu


def test_no_run_gives_zero_moments_and_touches_nothing_else():
    prop, almanac, central = leo_full_setup(degree=4)
    ctx = nx.GpuContext(prop.compile(almanac, central))
    try:
        lib = _abi.load_library()
        cap = 3
        runs, ref = _abi.TrajBatch(1, 4), _abi.TrajBatch(1, 4)               # (their arrays are not null; n = 0 of `runs` are read)
        ref.len[0] = 0
        values, length, epoch0 = np.full(6 * cap, 12345.0), np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int64)
        mom = np.full(cap * _abi.RIC_MOMENTS + 8, 12345.0)
        q = _abi.RicQuery()
        q.step_ns, q.frame_of, q.transport, q.smooth_window = 60 * nx.NS_PER_S, 1, 1, 5
        cin, cref = runs.as_c(), ref.as_c()
        rc = lib.nyx_hip_traj_ric_diff(ctx._h, C.byref(cin), 0, C.byref(cref), 1, C.byref(q), cap, values.ctypes.data_as(_abi.c_double_p),
                                       length.ctypes.data_as(_abi.c_int32_p), epoch0.ctypes.data_as(_abi.c_int64_p),
                                       mom.ctypes.data_as(_abi.c_double_p))
        assert rc == _abi.RC_OK, _abi.last_error()
        assert (mom[:cap * _abi.RIC_MOMENTS] == 0.0).all() and (mom[cap * _abi.RIC_MOMENTS:] == 12345.0).all()   # 3 x 28 zeros, nothing beyond
        assert (values == 12345.0).all() and length[0] == -7 and epoch0[0] == -7
        assert ctx.last_kernel_ms() >= 0.0                                   # the bracket's two events were recorded
    finally:
        ctx.close()

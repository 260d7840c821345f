"""When a frame takes the one-pass level 1 (gs_host::L1FusedPolicy in 3dgs.cpp_amd/csrc/gs_depth_policy.h) on the CPU: the test
plays the renderer (tests/native/l1_fused_policy_sim.cpp).  No reference counterpart: the reference sorts every instance globally.
The expected values follow from the rule as gs3d_hip.h states it: bin-local frames with bins of <= 8 x 8 tiles, scenes below the
dense-list threshold that have their spatial copy, a bin region (candidate capacity / bins) of at least 5/4 of the last retired
frame's fullest bin (or no frame of this shape retired yet), at most 8 bins per visible Gaussian, 32 frames of hold after a region
overflow, and a candidate buffer that may grow to 4 x its default size."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dgs.cpp_amd", "csrc")
ANY_ORDER, PLANES, SPATIAL = 1, 2, 4
ALL = ANY_ORDER | PLANES | SPATIAL
HD = (1920, 1080, 3)   # width, height, bin shift: 15 x 9 bins
BINS = 135
NAMES = ("engage", "switched_off", "not_any_order", "dense_regime", "no_spatial_copy", "held", "cap_too_small", "wide_splats")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("l1policy") / "libl1_fused_policy_sim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "l1_fused_policy_sim.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.lf_new.restype = C.c_void_p
    lib.lf_new.argtypes = [C.c_int]
    lib.lf_free.argtypes = [C.c_void_p]
    lib.lf_hold.restype = C.c_uint32
    lib.lf_hold.argtypes = [C.c_void_p]
    lib.lf_region_cap.restype = C.c_uint32
    lib.lf_region_cap.argtypes = [C.c_uint32, C.c_uint32]
    lib.lf_decide.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32]
    lib.lf_grow_to.restype = C.c_uint32
    lib.lf_grow_to.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.lf_retired.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.lf_region_overflowed.argtypes = [C.c_void_p]
    lib.lf_const.restype = C.c_uint32
    assert [lib.lf_const(k) for k in range(3)] == [32, 4, 8]
    return lib


class Policy:
    def __init__(self, lib, mode=-1):
        self.lib, self.h = lib, lib.lf_new(mode)
        self.verdicts = {lib.lf_verdict(k): NAMES[k] for k in range(len(NAMES))}

    def __del__(self):
        self.lib.lf_free(self.h)

    def decide(self, cand, flags=ALL, shape=HD, bins=BINS):
        return self.verdicts[self.lib.lf_decide(self.h, flags, shape[0], shape[1], shape[2], cand, bins)]

    def grow_to(self, cand, default, flags=ALL, shape=HD, bins=BINS):
        return self.lib.lf_grow_to(self.h, flags, shape[0], shape[1], shape[2], cand, bins, default)

    def retired(self, max_bin, e1=1500, v=1000, shape=HD, frames=1):
        for _ in range(frames):
            self.lib.lf_retired(self.h, shape[0], shape[1], shape[2], max_bin, e1, v)

    def overflowed(self):
        self.lib.lf_region_overflowed(self.h)

    @property
    def hold(self):
        return self.lib.lf_hold(self.h)


def test_engages_before_any_frame_has_retired(sim):
    assert sim.lf_region_cap(2_000_000, BINS) == 2_000_000 // BINS
    assert Policy(sim).decide(2_000_000) == "engage"


def test_refuses_by_structure(sim):
    p = Policy(sim)
    assert p.decide(2_000_000, flags=ALL & ~ANY_ORDER) == "not_any_order"    # global depth order, or bins beyond 8 x 8 tiles
    assert p.decide(2_000_000, flags=ALL & ~PLANES) == "dense_regime"        # a scene of dense_min Gaussians or more
    assert p.decide(2_000_000, flags=ALL & ~SPATIAL) == "no_spatial_copy"
    assert p.decide(BINS - 1) == "cap_too_small"                             # not one record per bin


def test_the_switch(sim):
    off, on = Policy(sim, mode=0), Policy(sim, mode=1)
    assert off.decide(2_000_000) == "switched_off"
    # forced on: wherever the frame's structure allows, whatever the scene's order and the last frame's counts ...
    on.retired(max_bin=10**6, e1=10**6, v=10)
    assert on.decide(2_000_000, flags=ANY_ORDER | PLANES) == "engage"
    # ... but never outside it
    assert on.decide(2_000_000, flags=PLANES | SPATIAL) == "not_any_order"
    assert on.decide(2_000_000, flags=ANY_ORDER | SPATIAL) == "dense_regime"


def test_the_five_quarters_edge(sim):
    p = Policy(sim)
    p.retired(max_bin=4000)                       # needs cap >= 5000
    assert p.decide(5000 * BINS) == "engage"      # cap == 5000: exactly 5/4
    assert p.decide(5000 * BINS - 1) == "cap_too_small"   # cap == 4999
    p.retired(max_bin=4001)                       # 5/4 of it = 5001.25
    assert p.decide(5001 * BINS) == "cap_too_small"
    assert p.decide(5002 * BINS) == "engage"


def test_another_shape_is_a_fresh_start(sim):
    p = Policy(sim)
    p.retired(max_bin=10**6)
    assert p.decide(2_000_000) == "cap_too_small"
    assert p.decide(2_000_000, shape=(1280, 720, 3), bins=60) == "engage"    # another resolution: its frame tells
    assert p.decide(2_000_000, shape=(1920, 1080, 2), bins=510) == "engage"  # the same resolution with smaller bins


def test_hold_after_an_overflow_then_the_rule_again(sim):
    p = Policy(sim)
    assert p.decide(2_000_000) == "engage"
    p.overflowed()
    assert p.hold == 32 and p.decide(2_000_000) == "held"
    assert Policy(sim, mode=1).decide(2_000_000) == "engage"
    forced = Policy(sim, mode=1)
    forced.overflowed()
    assert forced.decide(2_000_000) == "held"     # the hold binds the forced mode too: the re-run must not overflow again
    # the re-run frames retire on the three kernels and say what the fullest bin really holds
    cap = 2_000_000 // BINS
    p.retired(max_bin=cap, frames=31)
    assert p.hold == 1 and p.decide(2_000_000) == "held"
    p.retired(max_bin=cap)
    assert p.hold == 0
    assert p.decide(2_000_000) == "cap_too_small"      # re-engages only if the rule allows: cap < 5/4 of the fullest bin
    p.retired(max_bin=cap * 4 // 5)
    assert p.decide(2_000_000) == "engage"


def test_growth_and_its_ceiling(sim):
    p = Policy(sim)
    default = 2_000_000
    assert p.grow_to(default, default) == 0            # nothing retired yet: engaged, nothing to grow for
    p.retired(max_bin=20_000)                          # 5/4 -> 25 000 per bin, + a quarter of head-room -> 30 000
    assert p.decide(default) == "cap_too_small"
    want = p.grow_to(default, default)
    assert want == 30_000 * BINS and want <= 4 * default
    assert p.decide(want) == "engage"
    p.retired(max_bin=60_000)                          # 90 000 x 135 = 12.15 M > 4 x default: the frame stays as it is
    assert p.grow_to(default, default) == 0
    # exactly at the ceiling is allowed, one record beyond is not
    p.retired(max_bin=40_000)                          # 60 000 per bin
    assert p.grow_to(default, 60_000 * BINS // 4) == 60_000 * BINS
    assert p.grow_to(default, 60_000 * BINS // 4 - 1) == 0
    # only a region that is too small grows the buffer: never a hold, a switch, the scene's order or wide splats
    p.overflowed()
    assert p.grow_to(default, 60_000 * BINS) == 0
    assert Policy(sim, mode=0).grow_to(default, 10 * default) == 0
    q = Policy(sim)
    q.retired(max_bin=20_000)
    assert q.grow_to(default, default, flags=ALL & ~SPATIAL) == 0
    q.retired(max_bin=20_000, e1=9000, v=1000)
    assert q.decide(default) == "wide_splats" and q.grow_to(default, default) == 0


def test_wide_splats_leave_the_path(sim):
    p = Policy(sim)
    p.retired(max_bin=100, e1=8000, v=1000)            # 8 bins per visible Gaussian: still in
    assert p.decide(2_000_000) == "engage"
    p.retired(max_bin=100, e1=8001, v=1000)
    assert p.decide(2_000_000) == "wide_splats"
    p.retired(max_bin=100, e1=1500, v=1000)            # the three-kernel frames keep reporting E1 / V: back in when it falls
    assert p.decide(2_000_000) == "engage"
    p.retired(max_bin=0, e1=0, v=0)                    # an empty frame
    assert p.decide(2_000_000) == "engage"

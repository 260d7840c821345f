"""The depth-order level policy and the bin grid (3dgs.cpp_amd/csrc/gs_depth_policy.h) on the CPU: the test plays the renderer
and hands the policy the two counters it decides by -- `overflow` and `max_bin` -- of frames that overflowed or retired
(tests/native/depth_policy_sim.cpp).  No reference counterpart: the reference orders every frame globally.  The expected values
follow from the limits 4096 / 8192 / 12288 / 16384 / 65535 candidates per bin at level 0 .. 4 and the 7/8 hysteresis."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dgs.cpp_amd", "csrc")
FIELDS = ("sort_mode", "level", "refined", "settle_level", "frames_since_fallback", "slab_hold", "slab_clean_frames", "min_bin_shift")
HD, UHD = (1920, 1080), (3840, 2160)
WIDE = (4112, 256)  # 257 x 16 tiles: bins of 16 x 16 tiles (33 bins of 8 do not fit across), which cannot be halved
BIN_OVERFLOW = 2  # Counters::overflow bit 1: a bin outgrew the in-LDS order of its level (bit 0: a buffer's capacity)


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("policy") / "libdepth_policy_sim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "depth_policy_sim.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.dp_new.restype = C.c_void_p
    lib.dp_new.argtypes = [C.c_int, C.c_int]
    lib.dp_free.argtypes = [C.c_void_p]
    lib.dp_get.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.dp_set.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.dp_set_sort_mode.argtypes = [C.c_void_p, C.c_int]
    lib.dp_frame_level.argtypes = [C.c_void_p]
    lib.dp_geometry.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]
    lib.dp_can_refine.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.dp_overflowed.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]
    lib.dp_retired.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    lib.dp_retired_at.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int]
    assert [lib.dp_limit(lv) for lv in range(5)] == [4096, 8192, 12288, 16384, 65535]
    return lib


class Policy:
    def __init__(self, lib, sort_mode=0, min_bin_shift=3, **state):
        self.lib, self.h = lib, lib.dp_new(sort_mode, min_bin_shift)
        self.RERUN, self.BIN_TOO_FULL, self.TOO_CROWDED = (lib.dp_verdict(k) for k in range(3))
        if state:
            self.set(**state)

    def __del__(self):
        self.lib.dp_free(self.h)

    def state(self):
        v = (C.c_int64 * 8)()
        self.lib.dp_get(self.h, v)
        return dict(zip(FIELDS, v))

    def __getattr__(self, name):
        if name in FIELDS:
            return self.state()[name]
        raise AttributeError(name)

    def set(self, **kw):
        s = self.state()
        assert set(kw) <= set(FIELDS)
        s.update(kw)
        self.lib.dp_set(self.h, (C.c_int64 * 8)(*[int(s[k]) for k in FIELDS]))

    def frame_level(self):
        return self.lib.dp_frame_level(self.h)

    def geometry(self, size):
        """(bin shift, bins across, bins down, grid shift), or None for 'resolution too large'"""
        g = (C.c_int * 4)()
        return tuple(g) if self.lib.dp_geometry(self.h, size[0], size[1], g) else None

    def can_refine(self, size):
        return bool(self.lib.dp_can_refine(self.h, *size))

    def frame(self, max_bin, overflow=BIN_OVERFLOW, size=HD, level=None, bin_shift=None):
        """A queued frame: by default one that ran with the policy's current level and bins."""
        return (self.frame_level() if level is None else level, self.geometry(size)[0] if bin_shift is None else bin_shift,
                size[0], size[1], overflow, max_bin)

    def overflowed(self, *frames):
        flat = [w for f in frames for w in f]
        return self.lib.dp_overflowed(self.h, (C.c_uint32 * len(flat))(*flat), len(frames))

    def retired(self, max_bin, frames=1, level=None, size=None):
        for _ in range(frames):
            if size is None:
                self.lib.dp_retired(self.h, self.frame_level() if level is None else level, max_bin)
            else:
                self.lib.dp_retired_at(self.h, self.frame_level() if level is None else level, max_bin, self.geometry(size)[0])


# ---- geometry ----

def test_bin_grids(sim):
    p = Policy(sim)
    assert p.geometry(HD) == (3, 15, 9, 4)
    assert p.geometry(UHD) == (3, 30, 17, 5)
    assert p.geometry((16384, 16384))[:3] == (5, 32, 32)
    assert p.geometry((16400, 16)) is None  # "resolution too large for the tile binning"
    assert p.geometry((16, 16400)) is None


def test_min_bin_shift(sim):
    fine = Policy(sim, min_bin_shift=2)
    assert fine.geometry(HD)[0] == 2 and not fine.can_refine(HD)
    assert Policy(sim, min_bin_shift=5).geometry((640, 360))[0] == 5
    assert Policy(sim).can_refine(HD)


def test_refined_halves_the_bins_while_the_grid_fits(sim):
    p = Policy(sim, refined=True)
    assert p.geometry(HD) == (2, 30, 17, 5)
    assert not p.can_refine(HD)  # (already)
    # 240 x 135 tiles: bins of 4 x 4 tiles would be a 60-wide grid
    assert p.geometry(UHD)[0] == 3 and not Policy(sim).can_refine(UHD)
    # never below 4 x 4 tiles
    assert Policy(sim, min_bin_shift=2, refined=True).geometry(HD)[0] == 2
    # 640 x 360 with bins of 32 x 32 tiles asked for: 16 x 16 still fits
    assert Policy(sim, min_bin_shift=5, refined=True).geometry((640, 360))[0] == 4


# ---- climbing ----

def test_a_full_bin_climbs_to_the_level_its_size_asks_for(sim):
    p = Policy(sim, frames_since_fallback=9)
    assert p.overflowed(p.frame(5000)) == p.RERUN and p.level == 1 and p.frames_since_fallback == 0
    p = Policy(sim)
    assert p.overflowed(p.frame(13000)) == p.RERUN
    assert (p.level, p.refined) == (3, False)
    # a buffer's capacity alone (overflow bit 0) is not the policy's business
    p = Policy(sim, frames_since_fallback=9)
    assert p.overflowed(p.frame(13000, overflow=1)) == p.RERUN and p.state() == Policy(sim, frames_since_fallback=9).state()


def test_bins_are_refined_before_slabs_and_the_first_clean_frame_settles_the_level(sim):
    for max_bin, lands_at in ((3000, 0), (3584, 0), (3585, 1), (9000, 2), (12000, 3)):
        p = Policy(sim)
        assert p.overflowed(p.frame(20000)) == p.RERUN
        assert (p.refined, p.level, p.settle_level) == (True, 3, True) and p.geometry(HD)[0] == 2
        p.retired(max_bin)
        assert (p.level, p.settle_level, p.refined) == (lands_at, False, True), max_bin
    # a frame that ran at another level than the one the refinement jumped to does not settle it
    p = Policy(sim)
    p.overflowed(p.frame(20000))
    p.retired(3000, level=0)
    assert (p.level, p.settle_level) == (3, True)


def test_beyond_the_refined_bins(sim):
    p = Policy(sim, refined=True, level=3)
    assert p.overflowed(p.frame(30000)) == p.RERUN and p.level == 4 and p.slab_hold == 32
    p = Policy(sim, refined=True, level=3)
    assert p.overflowed(p.frame(70000)) == p.RERUN and p.level == 5
    # forced bin-local: an error, and nothing has moved
    before = dict(sort_mode=2, refined=True, level=3, frames_since_fallback=7, slab_clean_frames=3)
    p = Policy(sim, **before)
    assert p.overflowed(p.frame(70000)) == p.BIN_TOO_FULL
    assert p.state() == Policy(sim, **before).state()
    # where the grid cannot be refined the same sizes go straight to the slabs / the global path
    p = Policy(sim)
    assert p.overflowed(p.frame(20000, size=UHD)) == p.RERUN and (p.level, p.refined) == (4, False)


# ---- bins of 16 x 16 tiles or more: one kernel, 16384 at every bin-local level, no slabs ----

def test_a_large_bin_that_cannot_be_halved_goes_straight_to_the_global_path(sim):
    p = Policy(sim, frames_since_fallback=9, slab_clean_frames=5)
    assert p.geometry(WIDE) == (4, 17, 1, 5) and not p.can_refine(WIDE)
    assert p.overflowed(p.frame(20000, size=WIDE)) == p.RERUN
    # one re-run: not level 4 first (the same kernel with the same 16384), and nothing charged to the slabs
    assert p.state() == Policy(sim, level=5, slab_clean_frames=5).state()
    assert (p.slab_hold, p.slab_clean_frames, p.refined, p.settle_level) == (32, 5, False, False)
    # the same from a level the policy had climbed to on another frame size, level 4 included
    for lv in (1, 3, 4):
        p = Policy(sim, level=lv, slab_clean_frames=5)
        assert p.overflowed(p.frame(20000, size=WIDE)) == p.RERUN
        assert (p.level, p.slab_hold, p.slab_clean_frames) == (5, 32, 5), lv
    # bins of 32 x 32 tiles (8208 px: 513 tiles, 17 bins across, 33 of 16 would not fit) alike
    p = Policy(sim)
    assert p.geometry((8208, 256))[0] == 5 and not p.can_refine((8208, 256))
    assert p.overflowed(p.frame(16385, size=(8208, 256))) == p.RERUN and (p.level, p.slab_hold) == (5, 32)


def test_forced_bin_local_mode_reports_a_large_bin_as_too_full(sim):
    before = dict(sort_mode=2, frames_since_fallback=7, slab_clean_frames=3)
    p = Policy(sim, **before)
    assert p.overflowed(p.frame(20000, size=WIDE)) == p.BIN_TOO_FULL  # not TOO_CROWDED: no slab ever saw this bin
    assert p.state() == Policy(sim, **before).state()
    p = Policy(sim, sort_mode=2, level=4)
    assert p.overflowed(p.frame(20000, size=WIDE)) == p.BIN_TOO_FULL and (p.level, p.slab_hold) == (4, 32)


def test_a_large_bin_is_still_halved_first(sim):
    # GS_BIN_SHIFT=4 on a small frame: bins of 16 x 16 tiles that can be halved
    p = Policy(sim, min_bin_shift=4)
    assert p.geometry((512, 512)) == (4, 2, 2, 4) and p.can_refine((512, 512))
    assert p.overflowed(p.frame(20000, size=(512, 512))) == p.RERUN
    assert (p.refined, p.level, p.settle_level, p.slab_hold) == (True, 3, True, 32) and p.geometry((512, 512))[0] == 3
    # 32 x 32 -> 16 x 16, and a bin of those beyond 16384 then has the global path only
    p = Policy(sim, min_bin_shift=5)
    assert p.overflowed(p.frame(70000, size=(1024, 1024))) == p.RERUN
    assert (p.refined, p.level) == (True, 3) and p.geometry((1024, 1024))[0] == 4
    assert p.overflowed(p.frame(17600, size=(1024, 1024))) == p.RERUN and (p.level, p.slab_hold, p.slab_clean_frames) == (5, 32, 0)
    # the default bins of a frame up to 4096 px are untouched by any of this
    p = Policy(sim)
    assert p.overflowed(p.frame(20000, size=UHD)) == p.RERUN and (p.level, p.refined) == (4, False)


def test_large_bins_leave_the_global_path_only_for_what_their_kernel_holds(sim):
    """Without slabs below it, level 5 steps down when the fullest bin fits 7/8 of 16384 -- not 7/8 of the slabs' 65535, which
    would send a bin of 20000 back into the overflow it came from every 32 frames."""
    p = Policy(sim, level=5)
    p.retired(20000, frames=100, size=WIDE)
    assert (p.level, p.frames_since_fallback) == (5, 0)
    p.retired(16384 * 7 // 8, frames=31, size=WIDE)
    assert p.level == 5
    p.retired(16384 * 7 // 8, size=WIDE)
    assert p.level == 4
    # bins that have slabs: as before
    p = Policy(sim, level=5)
    p.retired(20000, frames=32, size=HD)
    assert p.level == 4


# ---- slab hold ----

def test_a_slab_failure_that_is_not_about_size_holds_the_global_path(sim):
    p = Policy(sim, refined=True, level=4, slab_clean_frames=5)
    assert p.overflowed(p.frame(30000)) == p.RERUN
    assert (p.level, p.slab_hold, p.slab_clean_frames) == (5, 64, 0)
    p.retired(30000, frames=63)
    assert p.level == 5
    p.retired(30000)
    assert p.level == 4
    # a bin beyond the slabs' 65535 is about size: no hold
    p = Policy(sim, refined=True, level=4)
    assert p.overflowed(p.frame(65536)) == p.RERUN and (p.level, p.slab_hold) == (5, 32)


def test_the_hold_doubles_up_to_8192(sim):
    p = Policy(sim, refined=True, level=4)
    holds = []
    for _ in range(10):
        assert p.overflowed(p.frame(30000)) == p.RERUN and p.level == 5
        holds.append(p.slab_hold)
        p.retired(30000, frames=p.slab_hold - 1)
        assert p.level == 5
        p.retired(30000)
        assert p.level == 4
    assert holds == [64, 128, 256, 512, 1024, 2048, 4096, 8192, 8192, 8192]


def test_forced_bin_local_mode_reports_crowded_depths(sim):
    p = Policy(sim, sort_mode=2, refined=True, level=4, frames_since_fallback=7, slab_clean_frames=5)
    assert p.overflowed(p.frame(30000)) == p.TOO_CROWDED
    # what was changed before the failure was found stays changed
    assert p.state() == Policy(sim, sort_mode=2, refined=True, level=4, frames_since_fallback=7, slab_hold=64, slab_clean_frames=0).state()


def test_64_clean_frames_on_the_slabs_reset_the_hold(sim):
    p = Policy(sim, refined=True, level=4)
    p.overflowed(p.frame(30000))
    p.set(level=4)
    p.retired(30000, frames=63)  # (beyond 7/8 of level 3's 16384: no step down meanwhile)
    assert (p.level, p.slab_hold) == (4, 64)
    p.retired(30000)
    assert (p.level, p.slab_hold) == (4, 32)


# ---- step-down ----

def test_32_fitting_frames_step_one_level_down(sim):
    bound = 8192 * 7 // 8  # 7/8 of level 1's limit
    p = Policy(sim, level=2)
    p.retired(bound, frames=31)
    assert p.level == 2
    p.retired(bound)
    assert p.level == 1 and p.frames_since_fallback == 0
    p = Policy(sim, level=2)
    p.retired(bound, frames=31)
    p.retired(bound + 1)
    p.retired(bound, frames=31)
    assert p.level == 2
    p.retired(bound)
    assert p.level == 1
    # all the way: 32 frames per level
    p = Policy(sim, level=3)
    p.retired(100, frames=3 * 32 - 1)
    assert p.level == 1
    p.retired(100)
    assert p.level == 0


def test_the_global_mode_never_moves_the_level(sim):
    p = Policy(sim, sort_mode=1, level=2, refined=True, settle_level=True)
    assert p.frame_level() == 5
    p.retired(0, frames=200)
    assert p.overflowed(p.frame(70000, overflow=1)) == p.RERUN
    assert p.state() == Policy(sim, sort_mode=1, level=2, refined=True, settle_level=True).state()


# ---- un-refine ----

def test_small_bins_that_stay_half_empty_go_back_to_the_default_bins(sim):
    p = Policy(sim, refined=True)
    p.retired(2048, frames=31)
    assert (p.refined, p.level) == (True, 0)
    p.retired(2048)
    assert (p.refined, p.level, p.frames_since_fallback) == (False, 3, 0) and p.geometry(HD)[0] == 3
    p = Policy(sim, refined=True)
    p.retired(2048, frames=31)
    p.retired(2049)
    p.retired(2048, frames=31)
    assert (p.refined, p.level) == (True, 0)
    p.retired(2048)
    assert (p.refined, p.level) == (False, 3)


# ---- stale frames ----

def test_frames_of_another_level_or_bin_size_say_nothing(sim):
    before = dict(level=1, frames_since_fallback=5)
    p = Policy(sim, **before)
    assert p.overflowed(p.frame(13000, level=0), p.frame(70000, level=0)) == p.RERUN  # queued before the climb to level 1
    assert p.state() == Policy(sim, **before).state()
    before = dict(level=3, refined=True, frames_since_fallback=5)
    p = Policy(sim, **before)
    assert p.overflowed(p.frame(20000, bin_shift=3)) == p.RERUN  # ran with the bins of before the refinement
    assert p.state() == Policy(sim, **before).state()
    # beside a current frame: neither their flag nor their fullest bin counts
    p = Policy(sim)
    assert p.overflowed(p.frame(5000), p.frame(60000, level=2), p.frame(60000, bin_shift=2)) == p.RERUN
    assert (p.level, p.refined) == (1, False)
    p = Policy(sim)
    assert p.overflowed(p.frame(5000, overflow=0), p.frame(60000, level=2)) == p.RERUN
    assert p.level == 0


# ---- gs_set_sort_path ----

def test_set_sort_mode_clears_level_refined_and_the_step_down_count_only(sim):
    p = Policy(sim, level=4, refined=True, settle_level=True, frames_since_fallback=11, slab_hold=256, slab_clean_frames=7)
    sim.dp_set_sort_mode(p.h, 2)
    assert p.state() == dict(sort_mode=2, level=0, refined=False, settle_level=True, frames_since_fallback=0, slab_hold=256,
                             slab_clean_frames=7, min_bin_shift=3)

"""The guarded blend's pair loop where its path changes (gs_blend.hip: GS_PAIR_GUARDED / GS_PAIR_SLOW).

The loop takes a pair on its FAST path -- accumulate, restore exec, next pair -- unless a lane's new T lies below slice_hi, the
first binary32 above the guard's slice (bit pattern 0x38D20000, 1.00434e-4); only then does it take render.comp:83's compare, the
slice compare and the bookkeeping of a break, in an out-of-line stub per unrolled copy.  The kept entries of a chunk are staged
right-aligned to a multiple of four and the loop counts groups of four, entered at the copy that fits.  So the scenes here put
the change of path at every position: the breaking pair in each of the four copies with every entry count mod 4, across the
64-entry chunk edge, a break of some pixels followed by entries the survivors must still accumulate, one pixel that outlives the
other 63, T exactly on the deciding edge and one binary32 below it, inside the slice with and without an event, and chunks that
keep 1 .. 5 entries.

Everything happens in tile (1, 1) of a 48 x 48 frame, mostly in its quadrant of pixels 24 .. 31 (limit_scenes.GUARD_QUADRANT).  A
scene is built from three kinds of splat: a BIG one (sigma 60 px around the quadrant's centre: the same alpha on every pixel of
the quadrant to 0.5 %), a BLOB (sigma 8 px: alpha clamps to 0.99 on its centre pixel and the four beside it, not further out) and
a DOT (limit_scenes._splats: 0.3 px^2, seen by its own pixel and, five times weaker, the four beside it).  Where a scene claims
that a pixel's T stands on a given value or that it breaks at a given entry, trace() restates render.comp for that pixel in the
reference's arithmetic over the oracle's own records and lists -- it must reproduce the oracle's pixel bit for bit -- and the
claim is asserted on the CPU (test_*_stands_where_it_claims, no GPU).

Every scene is then rendered twice, with lockstep off and on: exp mode 2 bit for bit against the oracle's image, and the default
mode within the guarded tolerance (helpers.assert_guarded_close).
"""
import numpy as np
import pytest

import limit_scenes as ls
from helpers import assert_guarded_close, assert_images_identical, oracle_frame

W = H = ls.GUARD_FRAME
FOCAL = W / (2.0 * np.tan(np.radians(ls.FOV) / 2.0))
SITE = (27, 27)
F32 = np.float32
SLICE_LO, SLICE_HI = 0x38D10000, 0x38D20000       # gs_blend.hip: kGuardSlice << 16, (kGuardSlice + 1) << 16
T_CUT = int(F32(0.0001).view(np.uint32))          # 0x38D1B717
# the guard's coarse window around 1e-4 (gs_blend.hip: kGuardLo, kGuardHi), in binary64: only used with a margin
_COARSE = 297.0 * 1.05 * 2.0e-7 + 4096 * 1.05 * (8.0e-8 + 2.3841858e-7)
COARSE_LO, COARSE_HI = 1e-4 * (1.0 - _COARSE), 1e-4 * (1.0 + _COARSE)


def _bits(x):
    return int(F32(x).view(np.uint32))


def _from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def _logit(p):
    return float(F32(np.log(p / (1.0 - p))))


OPAQUE = 30.0                                      # sigmoid(30) is 1 in binary32: alpha = min(0.99, exp(power))


# ------------------------------------------------------------------------------------------------ building
def big(opacity_logit, dc):
    return dict(px=27.5, py=27.5, sigma=60.0, logit=opacity_logit, dc=dc)


def blob(px, py, opacity_logit, dc):
    return dict(px=px, py=py, sigma=8.0, logit=opacity_logit, dc=dc)


def dot(px, py, opacity_logit, dc):
    return dict(px=px, py=py, sigma=None, logit=opacity_logit, dc=dc)


def records(entries):
    """The entries in list order (front to back): depth patterns 1000 apart, ids in the same order."""
    n = len(entries)
    bits = (ls.DEPTH_2 + np.arange(n, dtype=np.int64) * 1000).astype(np.uint32)
    px = np.asarray([e["px"] for e in entries], np.float64)
    py = np.asarray([e["py"] for e in entries], np.float64)
    rec = ls._splats(bits, None, None, W, H, logit=np.asarray([e["logit"] for e in entries], np.float32), pixel=(px, py))
    tz = bits.view(np.float32).astype(np.float64)
    for i, e in enumerate(entries):
        if e["sigma"] is not None:
            rec[i, 55:58] = np.log(e["sigma"] * tz[i] / FOCAL)
        rec[i, 6:9] = e["dc"]
    return rec


def _colour(i):
    """SH DC of filler i: distinct, all three channels visible."""
    return (1.0 + 0.5 * np.sin(0.7 * i), 1.0 + 0.5 * np.cos(1.3 * i), 1.0 + 0.5 * np.sin(2.1 * i + 1.0))


BRIGHT = (3.0, 3.0, 3.0)


# ------------------------------------------------------------------------------------------------ the reference's chain
def trace(oracle, ref, px, py):
    """render.comp for pixel (px, py) over the oracle's records and tile list, operation for operation in binary32 (gs_oracle.c:
    gso_render, the default reading).  Returns (steps, rgb): a step per entry that passes :68 and :78 -- (index in the tile's
    list, exp(power), test_T, did the pixel break there)."""
    t = (py // 16) * ((W + 15) // 16) + px // 16
    ids = ref["sorted_payload"][int(ref["boundaries"][2 * t]):int(ref["boundaries"][2 * t + 1])]
    T = F32(1.0)
    c = [F32(0.0)] * 3
    steps = []
    for k, g in enumerate(ids.tolist()):
        a = ref["attr"][g]
        co = a["conic_opacity"]
        dx, dy = a["uv"][0] - F32(px), a["uv"][1] - F32(py)
        power = F32(-0.5) * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy
        if power > 0 or power != power:
            continue
        e = F32(oracle.expf_libm(power))
        alpha = min(F32(0.99), co[3] * e)
        if alpha < F32(1.0) / F32(255.0):
            continue
        test_T = T * (F32(1.0) - alpha)
        brk = bool(test_T < F32(0.0001))
        steps.append((k, e, test_T, brk))
        if brk:
            break
        c = [c[i] + a["color_radii"][i] * alpha * T for i in range(3)]
        T = test_T
    assert all(isinstance(v, np.float32) for v in c) and isinstance(T, np.float32)
    return steps, np.asarray(c, np.float32)


def traced(oracle, ref, px, py):
    """trace(), checked: it is the oracle's own chain only if it gives the oracle's pixel bit for bit."""
    steps, rgb = trace(oracle, ref, px, py)
    assert np.array_equal(rgb.view(np.uint32), np.ascontiguousarray(ref["image"][py, px, :3]).view(np.uint32)), (px, py)
    return steps


def break_index(steps):
    return steps[-1][0] if steps and steps[-1][3] else None


def copy_of(list_length, index):
    """The unrolled copy (0 .. 3) that takes entry `index` of a list every entry of which the quadrant keeps: the chunk's kept
    entries are staged behind (-n) & 3 empty slots, n = the chunk's entries."""
    n = min(64, list_length - 64 * (index // 64))
    return (((-n) & 3) + index % 64) & 3


def list_length(ref):
    t = 1 * ((W + 15) // 16) + 1
    return int(ref["boundaries"][2 * t + 1]) - int(ref["boundaries"][2 * t])


_frames = {}


def frame(oracle, name, rec):
    """The oracle's frame of a scene, computed once."""
    if name not in _frames:
        _frames[name] = oracle_frame(oracle, rec, W, H)[2]
    return _frames[name]


# ------------------------------------------------------------------------------------------------ the scenes
PLUG_FILLERS = (0, 1, 2, 3, 4, 5, 6, 7, 61, 62, 63, 64, 65, 66)
FILLER = _logit(0.03)


def behind(f):
    """How many bright entries follow the plugs.  The loop's copies are counted from the chunk's END (the kept entries are staged
    right-aligned), so the copy that takes the breaking pair is set by what follows it in the chunk: 1 .. 4 entries, in step
    with f so that f = 0 .. 7 puts the break in every copy twice, under every list length mod 4."""
    return 1 + (f + f // 4) % 4 if f < 8 else 1 + f % 4


def plugs(f):
    """f faint fillers, two plugs of alpha 0.99 and behind(f) bright opaque entries that must not be seen, all BIG: every pixel of
    the tile breaks at the second plug, entry f + 1 of a list of f + 2 + behind(f).  (f = 0: T (1 - alpha) = fl(0.01 x 0.01) lies inside the guard's
    window on all 64 pixels -- more replays than a quadrant is allowed, so it is re-rendered with the reference's arithmetic;
    with f >= 1 the break is 3 % or more below 1e-4, outside the slice.)"""
    e = [big(FILLER, _colour(i)) for i in range(f)] + [big(OPAQUE, _colour(f)), big(OPAQUE, _colour(f + 1))]
    e += [big(_logit(0.9), BRIGHT)] * behind(f)
    return records(e)


PARTIAL_AT = (4, 5, 6, 7)


def partial(k):
    """k - 1 faint BIG fillers, then two opaque BLOBs on the site: the site's pixel and the four beside it break at the second one,
    entry k; the pixels further out survive (alpha 0.98 twice leaves T = 2e-4 two pixels away, more beyond) and accumulate the k + 2
    coloured BIG entries of opacity 0.3 that follow (6 .. 9: the break in another copy each time) -- during which the nearer of them break as well, pair after pair."""
    e = [big(FILLER, _colour(i)) for i in range(k - 1)] + [blob(SITE[0], SITE[1], OPAQUE, _colour(k))] * 2
    e += [big(_logit(0.3), _colour(20 + i)) for i in range(k + 2)]
    return records(e)


SURVIVOR_FILLERS = (9, 10, 11, 12)
SURVIVOR = (24, 24)


def one_survivor(nf):
    """Three layers of DOTs of opacity 0.97 on every pixel of the quadrant but its corner (24, 24): 189 entries, within which the
    63 pixels break one after the other (a pixel's own three leave 2.7e-5).  The corner sees the dots beside it at a fifth of their
    opacity and lives on alone through nf faint BIG fillers -- two groups of four and more -- until two plugs end it at entry
    189 + nf + 1; 1 + nf % 4 bright entries follow (the break in another copy each time)."""
    e = []
    for layer in range(3):
        for y in range(24, 32):
            for x in range(24, 32):
                if (x, y) != SURVIVOR:
                    e.append(dot(x, y, _logit(0.97), _colour(x + 8 * y + layer)))
    e += [big(FILLER, _colour(i)) for i in range(nf)] + [big(OPAQUE, _colour(1)), big(OPAQUE, _colour(2))] + [big(_logit(0.9), BRIGHT)] * (1 + nf % 4)
    return records(e)


COUNTS = (1, 2, 3, 4, 5)


def counts(n):
    """A chunk that keeps n entries: n BIG ones of opacity 0.3."""
    return records([big(_logit(0.3), _colour(i)) for i in range(n)])


# T on the deciding edge.  A stack of DOTs on the site: j faint fillers, two of opacity 0.9, then layers A and B whose logits are
# searched (below) so that the site's T after B has a bit pattern in [lo, hi]; 2 + j coloured layers of opacity 0.5 behind them (B in
# another copy with every j).
EDGES = {
    # name: (lo, hi, what the site's pixel does at B)
    "at_slice_hi": (SLICE_HI, SLICE_HI, "T = slice_hi exactly: not below it, the fast path"),
    "below_slice_hi": (SLICE_HI - 1, SLICE_HI - 1, "the largest binary32 below slice_hi: the stub; in the slice, above the coarse window, no break"),
    "slice_above_window": (_bits(1.0020e-4), _bits(1.0040e-4), "in the slice, above the coarse window: the stub, no break, no event"),
    "slice_below_window": (_bits(9.9670e-5), _bits(9.9800e-5), "in the slice, below the coarse window: the stub, a break, no event"),
    "in_window": (T_CUT - 16, T_CUT - 1, "a break within 16 binary32 steps of 1e-4: event, replay, re-entry"),
}
EDGE_CASES = [(name, 0) for name in EDGES if name != "in_window"] + [("in_window", j) for j in range(4)] + [("at_slice_hi", 2), ("below_slice_hi", 3)]
_STRONG = _logit(0.9)


def _edge_entries(j, logit_a, logit_b):
    x, y = SITE
    e = [dot(x, y, FILLER, _colour(i)) for i in range(j)] + [dot(x, y, _STRONG, _colour(10)), dot(x, y, _STRONG, _colour(11))]
    e += [dot(x, y, logit_a, _colour(12)), dot(x, y, logit_b, _colour(13))]
    return e + [dot(x, y, _logit(0.5), BRIGHT)] + [dot(x, y, _logit(0.5), _colour(14 + i)) for i in range(1 + j)]


def _opacities(oracle, logit_bits):
    """The oracle's activation of these logits (bit patterns)."""
    rec = np.zeros((len(logit_bits), 62), np.float32)
    rec[:, 54] = _from_bits(logit_bits)
    rec[:, 58] = 1.0
    return oracle.activate_records(rec)["scale_opacity"][:, 3].astype(np.float32)


_edges = {}


def edge(oracle, name, j):
    """(records, index of B in the list).  The geometry does not depend on the opacities, so exp(power) of A and B at the site and
    the site's T in front of A come from the chain of a first scene; the logits of A (1024 neighbours of 0.9's, as far as needed) and of B (600 around
    the value that would do in exact arithmetic) are then searched over their binary32 patterns with the reference's products."""
    if (name, j) in _edges:
        return _edges[(name, j)]
    lo, hi, _ = EDGES[name]
    first = records(_edge_entries(j, _STRONG, _STRONG))
    steps = trace(oracle, oracle_frame(oracle, first, W, H)[2], *SITE)[0]
    by_index = {s[0]: s for s in steps}
    ia, ib = j + 2, j + 3
    t_front, e_a, e_b = by_index[ia - 1][2], by_index[ia][1], by_index[ib][1]
    a_bits = _bits(_STRONG) + 3 * np.arange(1024, dtype=np.int64)
    alpha_a = np.minimum(F32(0.99), _opacities(oracle, a_bits) * e_a)
    t_a = t_front * (F32(1.0) - alpha_a)                           # (96,) binary32
    target = 0.5 * (float(_from_bits(lo)) + float(_from_bits(hi)))
    found = None
    for i in range(len(a_bits)):
        want = (1.0 - target / float(t_a[i])) / float(e_b)        # B's opacity, in exact arithmetic
        b_bits = _bits(np.log(want / (1.0 - want))) + np.arange(-300, 300, dtype=np.int64)
        alpha_b = np.minimum(F32(0.99), _opacities(oracle, b_bits) * e_b)
        t_b = (t_a[i] * (F32(1.0) - alpha_b)).astype(np.float32).view(np.uint32)
        hit = np.nonzero((t_b >= lo) & (t_b <= hi))[0]
        if len(hit):
            found = (int(a_bits[i]), int(b_bits[hit[0]]))
            break
    assert found is not None, f"no pair of logits puts T in [{lo:#x}, {hi:#x}]"
    rec = records(_edge_entries(j, float(_from_bits(found[0])), float(_from_bits(found[1]))))
    _edges[(name, j)] = (rec, ib)
    return _edges[(name, j)]


# ------------------------------------------------------------------------------------------------ on the CPU: the claims
def _all_kept(ref):
    """Every entry of tile (1, 1)'s list has alpha >= 1/255 on some pixel of the quadrant (binary64, with a margin): the quadrant
    keeps them all, so an entry's place in the list is its place in the wave's kept entries."""
    t = 1 * ((W + 15) // 16) + 1
    ids = ref["sorted_payload"][int(ref["boundaries"][2 * t]):int(ref["boundaries"][2 * t + 1])]
    a = ref["attr"][ids]
    ys, xs = np.mgrid[24:32, 24:32]
    dx = a["uv"][:, 0].astype(np.float64)[:, None] - xs.ravel()[None, :]
    dy = a["uv"][:, 1].astype(np.float64)[:, None] - ys.ravel()[None, :]
    co = a["conic_opacity"].astype(np.float64)
    power = -0.5 * (co[:, 0:1] * dx * dx + co[:, 2:3] * dy * dy) - co[:, 1:2] * dx * dy
    alpha = np.where(power <= 0, co[:, 3:4] * np.exp(np.minimum(power, 0.0)), 0.0)
    return bool((alpha.max(axis=1) > 1.05 / 255.0).all())


@pytest.mark.parametrize("f", PLUG_FILLERS)
def test_plugs_stand_where_they_claim(oracle, f):
    ref = frame(oracle, f"plugs/{f}", plugs(f))
    assert list_length(ref) == f + 2 + behind(f) and _all_kept(ref)
    for px, py in ((24, 24), (27, 27), (31, 24), (31, 31)):
        steps = traced(oracle, ref, px, py)
        assert break_index(steps) == f + 1 and len(steps) == f + 2
        assert all(int(s[2].view(np.uint32)) >= SLICE_HI for s in steps[:-1])         # fast path up to the break
        assert f == 0 or int(steps[-1][2].view(np.uint32)) < SLICE_LO                  # a plain break, below the slice
        assert f != 0 or COARSE_LO * 1.0001 < float(steps[-1][2]) < 1e-4               # (f = 0: inside the window)
    assert not ref["image"][24:32, 24:32, :3].max() > 1.3                               # the bright entries stayed unseen
    assert ref["image"][24:32, 24:32, :3].min() > 0


def test_plugs_put_the_break_in_every_copy_with_every_count():
    small = [(copy_of(f + 2 + behind(f), f + 1), (f + 2 + behind(f)) % 4) for f in range(8)]
    assert sorted(c for c, _ in small) == [0, 0, 1, 1, 2, 2, 3, 3] and {m for _, m in small} == {0, 1, 2, 3}
    # across the chunk edge: the break as the last pair of the first chunk (f = 62) and as the first of the next (f = 63)
    assert (62 + 1) % 64 == 63 and (63 + 1) % 64 == 0
    assert {copy_of(f + 2 + behind(f), f + 1) for f in (61, 62, 63, 64, 65, 66)} == {0, 1, 2, 3}


@pytest.mark.parametrize("k", PARTIAL_AT)
def test_partial_break_stands_where_it_claims(oracle, k):
    ref = frame(oracle, f"partial/{k}", partial(k))
    n = list_length(ref)
    assert n == 2 * k + 3 and _all_kept(ref)
    for px, py in (SITE, (26, 27), (27, 28)):
        assert break_index(traced(oracle, ref, px, py)) == k
    far = traced(oracle, ref, 24, 24)
    assert break_index(far) is None and len(far) == n                                   # a survivor takes every entry
    later = {break_index(traced(oracle, ref, px, py)) for px in range(24, 32) for py in range(24, 32)} - {None, k}
    assert later and min(later) > k                                                     # more breaks among the survivors


def test_partial_breaks_cover_every_copy():
    assert {copy_of(2 * k + 3, k) for k in PARTIAL_AT} == {0, 1, 2, 3}


@pytest.mark.parametrize("nf", SURVIVOR_FILLERS)
def test_one_survivor_stands_where_it_claims(oracle, nf):
    ref = frame(oracle, f"survivor/{nf}", one_survivor(nf))
    assert list_length(ref) == 189 + nf + 3 + nf % 4 and _all_kept(ref)
    for py in range(24, 32):
        for px in range(24, 32):
            at = break_index(traced(oracle, ref, px, py))
            if (px, py) == SURVIVOR:
                assert at == 189 + nf + 1
            else:
                assert at is not None and at < 189
    assert nf >= 9                                                                      # two groups of four and more, alone


def test_one_survivor_breaks_in_every_copy():
    assert {copy_of(189 + nf + 3 + nf % 4, 189 + nf + 1) for nf in SURVIVOR_FILLERS} == {0, 1, 2, 3}


@pytest.mark.parametrize("name,j", EDGE_CASES)
def test_edge_stands_where_it_claims(oracle, name, j):
    rec, ib = edge(oracle, name, j)
    ref = frame(oracle, f"edge/{name}/{j}", rec)
    lo, hi, _ = EDGES[name]
    assert list_length(ref) == 2 * j + 6 and _all_kept(ref)
    steps = {s[0]: s for s in traced(oracle, ref, *SITE)}
    t_b = int(steps[ib][2].view(np.uint32))
    assert lo <= t_b <= hi, f"{name}: T after B is {t_b:#x}"
    assert all(int(steps[i][2].view(np.uint32)) > SLICE_HI for i in range(ib))         # the fast path up to B
    assert steps[ib][3] == (name in ("slice_below_window", "in_window"))
    value = float(steps[ib][2])
    if name == "slice_above_window":
        assert value > COARSE_HI * 1.0001
    if name == "slice_below_window":
        assert value < COARSE_LO * 0.9999
    # the pixels beside the site see a fifth of every opacity: nowhere near the edge
    for px, py in ((26, 27), (27, 26), (28, 28)):
        assert all(float(s[2]) > 0.05 for s in traced(oracle, ref, px, py))


def test_in_window_events_cover_every_copy():
    assert {copy_of(2 * j + 6, j + 3) for j in range(4)} == {0, 1, 2, 3}


@pytest.mark.parametrize("n", COUNTS)
def test_counts_stand_where_they_claim(oracle, n):
    ref = frame(oracle, f"counts/{n}", counts(n))
    assert list_length(ref) == n and _all_kept(ref)
    assert len(traced(oracle, ref, 27, 27)) == n


# ------------------------------------------------------------------------------------------------ on the GPU
def _render_both(pkg, oracle, name, rec, lockstep):
    """Exp mode 2 bit for bit, the default mode within the guarded tolerance; returns the default mode's (redo, resolved)."""
    ref = frame(oracle, name, rec)
    gs = pkg.Scene.from_records(rec, device=0)
    rend = pkg.Renderer(gs)
    try:
        u = pkg.camera_uniforms(pkg.make_camera(), W, H)
        rend.set_blend_lockstep(lockstep)
        rend.set_exp_mode(2)
        img, _ = rend.render_host(u)
        label = f"{name} lockstep {lockstep}"
        assert_images_identical(img, ref["image"], label=label)
        worst, redo, resolved = assert_guarded_close(rend, u, ref["image"], label=f"{label}, default blend")
        print(f"{label}: default blend max |d| {worst:.3g}, quadrants re-rendered {redo}, breaks resolved {resolved}")
        return redo, resolved
    finally:
        rend.close()
        gs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("f", PLUG_FILLERS)
def test_every_pixel_breaks_at_the_same_entry(pkg, oracle, gpu, f, lockstep):
    # (the guard's counters are the whole frame's, and the BIG splats reach every tile with other alphas: nothing is asserted of them)
    _render_both(pkg, oracle, f"plugs/{f}", plugs(f), lockstep)


@pytest.mark.gpu
@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("k", PARTIAL_AT)
def test_partial_break_then_survivors_accumulate(pkg, oracle, gpu, k, lockstep):
    _render_both(pkg, oracle, f"partial/{k}", partial(k), lockstep)


@pytest.mark.gpu
@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("nf", SURVIVOR_FILLERS)
def test_one_pixel_outlives_the_quadrant(pkg, oracle, gpu, nf, lockstep):
    _render_both(pkg, oracle, f"survivor/{nf}", one_survivor(nf), lockstep)


@pytest.mark.gpu
@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("name,j", EDGE_CASES)
def test_T_at_the_deciding_edge(pkg, oracle, gpu, name, j, lockstep):
    rec, _ = edge(oracle, name, j)
    redo, resolved = _render_both(pkg, oracle, f"edge/{name}/{j}", rec, lockstep)
    assert redo == 0
    if name == "in_window":
        assert resolved > 0
    else:
        assert resolved == 0


@pytest.mark.gpu
@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("n", COUNTS)
def test_chunks_of_one_to_five_entries(pkg, oracle, gpu, n, lockstep):
    assert _render_both(pkg, oracle, f"counts/{n}", counts(n), lockstep) == (0, 0)

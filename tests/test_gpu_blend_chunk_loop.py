"""The blend's chunk loop (gs_blend.hip, blend_walk) after the entry-only terms of its quadrant test moved into the attribute record:
every (wave, chunk) must keep the entries it kept before, the prefetch must run off a list's end cleanly, a quadrant may leave the
loop in any chunk while its siblings walk on, the guard may give a quadrant up in any chunk, and the stage taps must find their
fields in the re-laid record.  Scenes: the helpers of tests/limit_scenes.py (tiny isotropic splats, identity camera, depths as bit
patterns); every frame is compared with the oracle, which culls nothing: the stage taps and the exp-mode-2 image bit for bit, the
default blend (mode 3) within the guarded tolerance.

tests/test_gpu_limits.py::test_blend_list_lengths_around_the_chunks covers lists of 1 .. 193 entries; this file goes on from there."""
import numpy as np
import pytest

import limit_scenes as ls
from helpers import assert_guarded_close, assert_images_identical, compare_stages, oracle_frame

pytestmark = pytest.mark.gpu

CHUNK = ls.BLEND_CHUNK


def _open(pkg, oracle, monkeypatch, rec, w, h):
    monkeypatch.delenv("GS_SORT_PATH", raising=False)
    verts, u_ref, ref = oracle_frame(oracle, rec, w, h)
    gs = pkg.Scene.from_records(rec, device=0)
    u = pkg.camera_uniforms(pkg.make_camera(), w, h)
    assert u.tobytes() == u_ref.tobytes()
    return gs, pkg.Renderer(gs), u, ref, verts


def _assert_frame(pkg, rend, u, ref, label):
    """Taps and the mode-2 image exact, the default blend within the guarded tolerance; returns (redo, resolved) of the latter."""
    img, _ = rend.render_host(u)
    compare_stages(pkg, rend, u, ref)
    assert_images_identical(img, ref["image"], label=label)
    worst, redo, resolved = assert_guarded_close(rend, u, ref["image"], label=f"{label}, default blend")
    print(f"{label}: default blend max |d| {worst:.3g}, quadrants re-rendered {redo}, breaks resolved {resolved}")
    return redo, resolved


def _tile_list(ref, w, tile):
    t = tile[1] * ls.tiles_across(w) + tile[0]
    b = ref["boundaries"].astype(np.int64)
    return ref["sorted_payload"][b[2 * t]:b[2 * t + 1]]


# ------------------------------------------------------------------------------------------------ list lengths
LENGTHS = (255, 256, 257, 319, 320, 321)


def _two_lists(k):
    """limit_scenes.blend_chunk for longer lists: tile (2, 1) of a 96 x 64 frame holds exactly k entries, its right neighbour the
    next length; opacity 0.02, so no pixel stops early (0.98^321 = 1.5e-3) and every entry of either list is walked."""
    w, h = 96, 64
    other = LENGTHS[(LENGTHS.index(k) + 1) % len(LENGTHS)]
    n = k + other
    ids = (np.arange(n, dtype=np.int64) * 13) % n
    rec = ls._splats(ls._spread_bits(n), np.where(ids >= k, 3, 2), np.ones(n), w, h, logit=np.log(0.02 / 0.98))
    return rec, w, h, other


@pytest.mark.parametrize("lockstep", [0, 1])
@pytest.mark.parametrize("k", LENGTHS)
def test_lists_that_end_around_the_fourth_and_fifth_chunk(pkg, oracle, gpu, monkeypatch, k, lockstep):
    """Lists one short of four and five whole chunks, on them and one beyond: the record prefetch (one chunk ahead) and the id
    prefetch (two ahead) run off the list's end in an even and in an odd chunk, with a ragged, a full and a one-entry last chunk."""
    rec, w, h, other = _two_lists(k)
    gs, rend, u, ref, _ = _open(pkg, oracle, monkeypatch, rec, w, h)
    try:
        assert len(_tile_list(ref, w, (2, 1))) == k and len(_tile_list(ref, w, (3, 1))) == other
        rend.set_blend_lockstep(lockstep)
        _assert_frame(pkg, rend, u, ref, f"list of {k}, lockstep {lockstep}")
        assert rend.stats().num_instances == k + other
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ quadrants that end early
def _break_positions(ref, w, tile):
    """Per pixel of a tile: the position in the tile's list at which render.comp:83 breaks (float64 re-trace), or -1."""
    ids = _tile_list(ref, w, tile)
    a = ref["attr"][ids]
    co = a["conic_opacity"].astype(np.float64)
    out = np.full((16, 16), -1, np.int64)
    for py in range(16):
        for px in range(16):
            dx = a["uv"][:, 0].astype(np.float64) - (tile[0] * 16 + px)
            dy = a["uv"][:, 1].astype(np.float64) - (tile[1] * 16 + py)
            power = -0.5 * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy
            alpha = np.minimum(0.99, co[:, 3] * np.exp(np.minimum(power, 0.0)))
            T = 1.0
            for j in np.nonzero((power <= 0) & (alpha >= 1.0 / 255.0))[0]:
                T *= 1.0 - alpha[j]
                if T < 1e-4:
                    out[py, px] = j
                    break
    return out


def _saturated_quadrant(chunk, quadrant, n_weak=5 * CHUNK + 8, layers=8, sigma_px=6.0):
    """Tile (1, 1) of a 64 x 64 frame: n_weak faint splats (the list: more than five chunks) and, at list positions inside `chunk`,
    `layers` opaque splats six pixels wide on the centre of one quadrant -- every pixel of that quadrant saturates inside that
    chunk, while every other quadrant of the tile keeps pixels that never do and walks the whole list."""
    w = h = 64
    weak = ls._splats(ls._spread_bits(n_weak), np.ones(n_weak), np.ones(n_weak), w, h, logit=np.log(0.02 / 0.98))
    stride = (1 << 23) // n_weak
    bits = (ls.DEPTH_2 + (CHUNK * chunk + 20 + np.arange(layers)) * stride + stride // 2).astype(np.uint32)
    cx, cy = 16 + 8 * (quadrant & 1) + 3.5, 16 + 8 * (quadrant >> 1) + 3.5
    big = ls._splats(bits, None, None, w, h, logit=12.0, pixel=(np.full(layers, cx), np.full(layers, cy)))
    focal = w / (2.0 * np.tan(np.radians(ls.FOV) / 2.0))
    big[:, 55:58] = np.log(sigma_px * bits.view(np.float32).astype(np.float64) / focal)[:, None]
    return np.concatenate([weak, big]), w, h


@pytest.mark.parametrize("quadrant", [0, 3])
@pytest.mark.parametrize("chunk", [1, 2, 3])
def test_a_quadrant_that_saturates_in_chunk_one_two_or_three_while_its_siblings_walk_on(pkg, oracle, gpu, monkeypatch, chunk, quadrant):
    """Lockstep on: the wave that leaves the loop in an odd or an even chunk no longer counts for the barrier its three siblings
    keep taking to the end of a list of more than five chunks."""
    rec, w, h = _saturated_quadrant(chunk, quadrant)
    gs, rend, u, ref, _ = _open(pkg, oracle, monkeypatch, rec, w, h)
    try:
        assert len(_tile_list(ref, w, (1, 1))) > 5 * CHUNK
        pos = _break_positions(ref, w, (1, 1))
        for q in range(4):
            blk = pos[8 * (q >> 1):8 * (q >> 1) + 8, 8 * (q & 1):8 * (q & 1) + 8]
            if q == quadrant:   # its last pixel stops inside the chunk, well away from the chunk's ends
                assert (blk >= 0).all() and CHUNK * chunk + 8 <= blk.max() < CHUNK * (chunk + 1) - 8, (q, blk.max())
            else:
                assert (blk < 0).sum() >= 32, (q, int((blk < 0).sum()))
        rend.set_blend_lockstep(1)
        _assert_frame(pkg, rend, u, ref, f"quadrant {quadrant} saturates in chunk {chunk}")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ the guard gives up, in any chunk
_guard_scenes = {}


def _front(count):
    """`count` splats of tile (1, 1) of the guard scenes' frame, in front of everything else and on a pixel of the tile's FIRST
    quadrant: the quadrant under test (the fourth) culls them, so they move its kept entries `count` places down the list."""
    if count == 0:
        return np.zeros((0, ls.RECORD_FLOATS), np.float32)
    return ls._splats(ls._spread_bits(count, lo=0x3FC00000, span=1 << 20), None, None, ls.GUARD_FRAME, ls.GUARD_FRAME,
                      logit=np.log(0.02 / 0.98), pixel=(np.full(count, 18.0), np.full(count, 18.0)))


def _behind(count):
    """`count` faint splats behind everything else, on a pixel of the quadrant under test two pixels from the nearest site: the
    quadrant keeps them, so there is a chunk after the one in which the guard made up its mind."""
    return ls._splats(ls._spread_bits(count, lo=0x40C00000, span=1 << 20), None, None, ls.GUARD_FRAME, ls.GUARD_FRAME,
                      logit=np.log(0.02 / 0.98), pixel=(np.full(count, 31.0), np.full(count, 27.0)))


def _guard_scene(oracle, kind):
    if kind not in _guard_scenes:
        image_of = lambda rec: oracle_frame(oracle, rec, ls.GUARD_FRAME, ls.GUARD_FRAME)[2]["image"]
        _guard_scenes[kind] = ls.guard_resolves(9, image_of) if kind == "replays" else ls.guard_pairs(ls.GUARD_PAIRS + 1)
    return _guard_scenes[kind]


@pytest.mark.parametrize("shift", [0, CHUNK], ids=["as_built", "one_chunk_later"])
@pytest.mark.parametrize("kind", ["replays", "pairs"])
def test_the_guard_gives_a_quadrant_up_in_an_even_and_in_an_odd_chunk(pkg, oracle, gpu, monkeypatch, kind, shift):
    """The ninth replay of a quadrant, and its 4097th kept entry, in chunks of either parity (64 entries of another quadrant in
    front of the list move everything one chunk on), with kept entries behind them: blend_redo counts the quadrant, which is then
    the reference's bit for bit."""
    scene = _guard_scene(oracle, kind)
    n0 = len(scene.records)
    rec = np.concatenate([scene.records, _front(shift), _behind(CHUNK + 6)])
    gs, rend, u, ref, _ = _open(pkg, oracle, monkeypatch, rec, ls.GUARD_FRAME, ls.GUARD_FRAME)
    try:
        ids = _tile_list(ref, ls.GUARD_FRAME, (1, 1))
        mine = np.nonzero(ids < n0)[0]                      # list positions of the quadrant's own entries, in list order
        if kind == "replays":
            decided = int(np.nonzero(np.isin(ids, scene.guard["last_ids"]))[0].max())   # the ninth break decision
        else:
            decided = int(mine[ls.GUARD_PAIRS])             # the 4097th kept entry
        assert (decided // CHUNK) % 2 == ((5 if kind == "replays" else 64) + shift // CHUNK) % 2
        assert len(ids) > (decided // CHUNK + 1) * CHUNK    # a later chunk exists
        _assert_frame(pkg, rend, u, ref, f"guard {kind}, {shift} in front")
        rend.set_exp_mode(3)
        rend.set_blend_contraction(False)
        img, _ = rend.render_host(u)
        st = rend.stats()
        rend.set_exp_mode(2)
        assert st.blend_redo == 1, f"quadrants re-rendered: {st.blend_redo}"
        q = ls.GUARD_QUADRANT
        assert np.array_equal(img[q][..., :3].view(np.uint32), np.ascontiguousarray(ref["image"][q][..., :3]).view(np.uint32))
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ the quadrant test is exact
def _grazing_scene():
    """A 64 x 64 frame.  (a) Tiny isotropic splats (conic 1 / 0.3) at the distance from a quadrant's edge or corner pixel at which
    alpha there equals 1/255, times 1 +- 1e-6 .. 1e-1: the alpha-cut ellipse grazes the quadrant from inside and just misses it.
    (b) Thin needles at 45 degrees, dozens of pixels long, whose axis passes a quadrant's corner pixel at a fraction of a pixel:
    the three terms of `power` are ~1e3 and cancel.  (c) Splats centred exactly on corner pixels of quadrants."""
    w = h = 64
    px, py, logit, target = [], [], [], []
    eps = np.array([s * 10.0 ** -e for e in (6, 5, 4, 3, 2, 1) for s in (-1, 1)])
    for x0, y0 in ((8, 8), (16, 24), (40, 16), (24, 40)):           # the quadrant's first pixel
        for ex, ey in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)):
            for k, o in enumerate((0.9, 0.3, 0.99995)):
                d = np.sqrt(2.0 * 0.3 * np.log(255.0 * o)) * (1.0 + eps[k::3])
                bx = x0 + (7 if ex > 0 else 0 if ex < 0 else 2 + k)    # the quadrant's pixel nearest to the splat
                by = y0 + (7 if ey > 0 else 0 if ey < 0 else 5 - k)
                norm = np.hypot(ex, ey)
                px += list(bx + ex / norm * d)
                py += list(by + ey / norm * d)
                logit += [np.log(o / (1.0 - o))] * len(d)
                target += [(bx, by)] * len(d)
    n_graze = len(px)
    needle_off = np.array([-0.9, -0.5, -0.2, -0.05, 0.0, 0.05, 0.2, 0.5, 0.9])
    for x0, y0 in ((16, 16), (32, 24), (24, 40)):
        for along in (12.0, 20.0, 28.0):                             # the centre this far along the axis from the corner pixel
            for sgn in (-1.0, 1.0):
                px += list(x0 + sgn * along / np.sqrt(2.0) + needle_off / np.sqrt(2.0))
                py += list(y0 + sgn * along / np.sqrt(2.0) - needle_off / np.sqrt(2.0))
                logit += [3.0] * len(needle_off)
    n_needle = len(px) - n_graze
    for x0 in (8, 15, 16, 23, 32, 39):
        for y0 in (8, 23, 40):
            px.append(float(x0))
            py.append(float(y0))
            logit.append(2.0)
    n = len(px)
    rec = ls._splats(ls._spread_bits(n), None, None, w, h, logit=np.asarray(logit), pixel=(np.asarray(px), np.asarray(py)))
    needles = slice(n_graze, n_graze + n_needle)
    tz = rec[needles, 2].astype(np.float64) * -1.0
    focal = w / (2.0 * np.tan(np.radians(ls.FOV) / 2.0))
    rec[needles, 55] = np.log(25.0 * tz / focal)                     # 25 px along, 0.55 px (the dilation) across
    rec[needles, 58] = np.cos(np.pi / 8.0)                           # 45 degrees about the view axis
    rec[needles, 61] = np.sin(np.pi / 8.0)
    return rec, w, h, n_graze, n_needle, np.asarray(target, np.float64)


def _assert_grazing(ref, target):
    """The scene stands where it should: at the pixel of the quadrant each isotropic splat was aimed at, alpha is within 2 % of
    1/255 for at least half of them, a quarter on either side."""
    a = ref["attr"][:len(target)]
    dx, dy = a["uv"][:, 0].astype(np.float64) - target[:, 0], a["uv"][:, 1].astype(np.float64) - target[:, 1]
    co = a["conic_opacity"].astype(np.float64)
    power = -0.5 * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy
    r = np.minimum(0.99, co[:, 3] * np.exp(power)) * 255.0
    below, above = int(((r > 0.98) & (r < 1.0)).sum()), int(((r >= 1.0) & (r < 1.02)).sum())
    assert below >= len(target) // 4 and above >= len(target) // 4, (below, above, len(target))


def test_the_quadrant_test_keeps_every_entry_a_pixel_keeps(pkg, oracle, gpu, monkeypatch):
    rec, w, h, n_graze, n_needle, target = _grazing_scene()
    assert 250 <= n_graze <= 600 and n_needle >= 100
    gs, rend, u, ref, _ = _open(pkg, oracle, monkeypatch, rec, w, h)
    try:
        _assert_grazing(ref, target)
        for lockstep in (0, 1):
            rend.set_blend_lockstep(lockstep)
            _assert_frame(pkg, rend, u, ref, f"grazing splats, lockstep {lockstep}")
    finally:
        rend.close()
        gs.close()


def test_the_quadrant_test_with_the_antialiased_opacity(pkg, oracle, gpu, monkeypatch):
    """The antialiased mode scales the opacity per frame and takes its alpha cut in k_preprocess: the frame is the oracle's frame
    of the scene that carries those opacities (tests/test_gpu_antialiased.py), bit for bit, grazing splats included."""
    rec, w, h, _, _, _ = _grazing_scene()
    gs, rend, u, _, verts = _open(pkg, oracle, monkeypatch, rec, w, h)
    try:
        rend.set_antialiased(True)
        img, _ = rend.render_host(u)
        vis = rend.stage("tiles") != 0
        prime = verts.copy()
        prime["scale_opacity"][vis, 3] = rend.stage("conic_opacity").reshape(-1, 4)[vis, 3]
        assert (prime["scale_opacity"][vis, 3] < verts["scale_opacity"][vis, 3]).mean() > 0.9
        ref = oracle.stages(prime, u.view(oracle.UNIFORMS_DT))
        assert_images_identical(img, ref["image"], label="grazing splats, antialiased")
        compare_stages(pkg, rend, u, ref)
        np.testing.assert_array_equal(rend.stage("alpha_cut")[vis].view(np.uint32),
                                      oracle.alpha_cut(prime["scale_opacity"][:, 3])[vis].view(np.uint32))
        assert_guarded_close(rend, u, ref["image"], label="grazing splats, antialiased, default blend")
    finally:
        rend.close()
        gs.close()


# ------------------------------------------------------------------------------------------------ the taps of the re-laid record
def test_the_record_taps_read_their_own_fields(pkg, oracle, gpu, monkeypatch):
    """radius, b, alpha cut and depth of every visible Gaussian, each against the oracle's own buffer -- and no two of the four
    hold the same numbers, so a tap that reads a neighbour's place fails here."""
    rec = pkg.synth.synth_records(3000, seed=5, kind="A")
    w, h = 160, 96
    gs, rend, u, ref, verts = _open(pkg, oracle, monkeypatch, rec, w, h)
    try:
        rend.render_host(u)
        vis = ref["tiles"] != 0
        assert vis.sum() > 1000 and np.array_equal(rend.stage("tiles"), ref["tiles"])
        attr = ref["attr"]
        want = dict(radius=attr["color_radii"][vis, 3], b=np.ascontiguousarray(attr["color_radii"][vis, 2]),
                    alpha_cut=oracle.alpha_cut(verts["scale_opacity"][:, 3])[vis], depth=attr["depth"][vis])
        for name, values in want.items():
            np.testing.assert_array_equal(rend.stage(name)[vis].view(np.uint32), values.astype(np.float32).view(np.uint32), err_msg=name)
        names = list(want)
        for i, p in enumerate(names):
            for q in names[i + 1:]:
                assert (want[p].astype(np.float32) != want[q].astype(np.float32)).mean() > 0.9, (p, q)
    finally:
        rend.close()
        gs.close()

"""Shared helpers for the parity tests: oracle <-> device layout conversion."""
import numpy as np


def assert_value_is_frames_over_time(line, rel=1e-5):
    """The bench line's identity `value == n_gpus * 1e3 / ms_per_step` (whole-job frames over the wall time of the median
    batch), with a tolerance that knows the quantum of what is printed: both numbers are written with >= 6 significant
    digits, so the identity holds to 1e-5 at ANY rate.  (Round 5 asserted 1e-3 against an `ms_per_step` of four decimals: a
    30 k-Gaussian scene at 21 120 frames/s broke it by rounding alone, and -- sorted first under `-x` -- that one harness
    assertion kept 250 kernel-parity tests from running on the driver's box.)"""
    v, ms, g = line["value"], line["ms_per_step"], line["n_gpus"]
    assert v > 0 and ms > 0
    assert abs(v - g * 1e3 / ms) / v < rel, (v, ms, g)


def oracle_frame(oracle, records, width, height, camera=None):
    verts = oracle.activate_records(records)
    cam = camera if camera is not None else oracle.default_camera()
    u = oracle.camera_uniforms(cam, width, height)
    return verts, u, oracle.stages(verts, u)


def expected_depth_order(attr, tiles):
    """Visible Gaussian ids ascending by (bits(depth), id) -- what a stable sort of the reference's
    64-bit keys implies inside every tile."""
    vis = np.nonzero(tiles)[0].astype(np.uint32)
    bits = attr["depth"][vis].view(np.uint32)
    order = np.lexsort((vis, bits))
    return vis[order]


def compare_stages(pkg, rend, u, ref):
    """Bit-exact comparison of every stage tap with the oracle's buffers."""
    attr, tiles = ref["attr"], ref["tiles"]
    vis = tiles != 0
    np.testing.assert_array_equal(rend.stage("tiles"), tiles)
    np.testing.assert_array_equal(rend.stage("depth")[vis].view(np.uint32), attr["depth"][vis].view(np.uint32))
    np.testing.assert_array_equal(rend.stage("radius")[vis], attr["color_radii"][vis, 3])
    np.testing.assert_array_equal(rend.stage("aabb").reshape(-1, 4)[vis], attr["aabb"][vis].astype(np.uint16))
    np.testing.assert_array_equal(rend.stage("conic_opacity").reshape(-1, 4)[vis].view(np.uint32),
                                  attr["conic_opacity"][vis].view(np.uint32))
    uv_rg = rend.stage("uv_rg").reshape(-1, 4)[vis]
    np.testing.assert_array_equal(uv_rg[:, :2].view(np.uint32), np.ascontiguousarray(attr["uv"][vis]).view(np.uint32))
    np.testing.assert_array_equal(uv_rg[:, 2:].view(np.uint32),
                                  np.ascontiguousarray(attr["color_radii"][vis, :2]).view(np.uint32))
    np.testing.assert_array_equal(rend.stage("b")[vis].view(np.uint32),
                                  np.ascontiguousarray(attr["color_radii"][vis, 2]).view(np.uint32))
    st = rend.stats()
    if st.sort_path == 1:  # the global depth order exists as a buffer on that path only (gs_set_sort_path)
        order = expected_depth_order(attr, tiles)
        np.testing.assert_array_equal(rend.stage("depth_order"), order)
    assert st.num_visible == int(vis.sum())
    assert st.num_instances == len(ref["keys"])
    np.testing.assert_array_equal(rend.stage("sorted_tile"), (ref["sorted_keys"] >> np.uint64(32)).astype(np.uint32))
    np.testing.assert_array_equal(rend.stage("sorted_gid"), ref["sorted_payload"])
    np.testing.assert_array_equal(rend.stage("ranges", u), ref["boundaries"])


# ---------------------------------------------------------------- image comparison across exp() implementations
# The DEFAULT blend (product and oracle) is bit-identical to the reference text compiled for the CPU: those comparisons
# are assert_array_equal on the bit patterns and need none of this.  What follows serves the OPT-IN fast modes
# (gs_set_exp_mode 0 / 1, gs_set_blend_contraction 1), whose difference from the reference text is characterised here:
# render.comp:77 leaves exp() to the implementation (GLSL: 3 + 2|x| ULP) and :66/:87 may or may not be contracted
# to FMAs.  Two conformant evaluations of the same lists therefore agree to a few ULP per pixel -- except where an
# entry's alpha falls within rounding of the 1/255 cut (render.comp:78), its power within rounding of 0 (:68), or
# the running transmittance within rounding of 1e-4 (:83): there the discrete decision can flip and the pixel moves
# by up to alpha * T * rgb ~ 4e-3.  classify_pixel() re-traces one pixel in float64 and reports how close its list
# comes to each threshold, so that a test can demand that EVERY pixel beyond ULP noise is such a flip, and count them.
ULP_NOISE = 1e-5        # measured 3e-7 .. 2e-6; anything above this must be an explained threshold flip
ALPHA_REL = 4e-6        # |alpha * 255 - 1| below this: alpha is within a few ULP of exp()/power of the cut
T_REL = 2e-4            # |T' / 1e-4 - 1|: T is a product of up to thousands of factors, each a few ULP apart
POWER_REL = 4e-6        # |power| relative to its terms
# Contraction sensitivity.  `power` is a sum of three products; when they cancel (a splat seen far from its centre along its
# long axis) one rounding more or less -- a contracted multiply-add, which GLSL permits and the pipeline makes, against the
# uncontracted evaluation of the reference text compiled for the CPU -- moves `power` by ~2^-24 x |terms|, alpha by alpha x
# that, and the pixel by T x alpha x that x |rgb|, thresholds or not.  classify_pixel() therefore (a) widens the distances
# to the alpha and T cuts by CANCEL_SLACK x that much, and (b) sums the first-order bound of the pixel's movement over the
# pixel's list ("cancel"): a pixel within CANCEL_SLACK x the bound is explained without any flip.
CANCEL_SLACK = 4.0


def classify_pixel(attr, boundaries, payload, width, px, py):
    tx = (width + 15) // 16
    t = (py // 16) * tx + (px // 16)
    ids = payload[boundaries[2 * t]:boundaries[2 * t + 1]]
    a = attr[ids]
    dx = a["uv"][:, 0].astype(np.float64) - px
    dy = a["uv"][:, 1].astype(np.float64) - py
    co = a["conic_opacity"].astype(np.float64)
    t1, t2, t3 = co[:, 0] * dx * dx, co[:, 2] * dy * dy, co[:, 1] * dx * dy
    power = -0.5 * (t1 + t2) - t3
    mag = 0.5 * (np.abs(t1) + np.abs(t2)) + np.abs(t3) + 1e-300
    alpha = np.minimum(0.99, co[:, 3] * np.exp(np.minimum(power, 0.0)))
    near = dict(alpha=np.inf, power=np.inf, T=np.inf, cancel=0.0)
    rgb = np.abs(a["color_radii"][:, :3].astype(np.float64)).max(axis=1)
    T = 1.0
    t_err = 0.0  # relative uncertainty of the running transmittance from the cancellation in the entries so far
    for k in range(len(ids)):
        near["power"] = min(near["power"], abs(power[k]) / mag[k] if mag[k] > 1e-30 else np.inf)
        if power[k] > 0:
            continue
        d_power = CANCEL_SLACK * 2.0 ** -24 * mag[k]  # how far one rounding of the largest term can move `power`
        # distances to the cuts, less what the cancellation alone can move alpha / T by (relative): 0 = may flip
        near["alpha"] = min(near["alpha"], max(0.0, abs(alpha[k] * 255.0 - 1.0) - d_power))
        if alpha[k] < 1.0 / 255.0:
            continue
        test_T = T * (1.0 - alpha[k])
        t_err += d_power * alpha[k] / max(1.0 - alpha[k], 1e-2)
        near["T"] = min(near["T"], max(0.0, abs(test_T / 1e-4 - 1.0) - t_err))
        if test_T < 1e-4:
            break
        # this entry's contribution and everything behind it move by at most T x alpha x d_power x max(1, |rgb|)
        near["cancel"] += T * alpha[k] * 2.0 ** -24 * mag[k] * max(1.0, rgb[k])
        T = test_T
    return near


HOST_LIBM_MISMATCHES = 0  # set by conftest's oracle fixture: sampled disagreements between the restated expf and this host's libm


def assert_images_identical(img, ref_img, label=""):
    """Bit-for-bit equality of two fp32 images (the exact blend against the reference text / the oracle)."""
    a, b = np.ascontiguousarray(img, np.float32).view(np.uint32), np.ascontiguousarray(ref_img, np.float32).view(np.uint32)
    if not np.array_equal(a, b) and HOST_LIBM_MISMATCHES:
        import pytest
        # a foreign libm explains last-bit differences of exp(), nothing larger: wrong lists, a wrong blend or a permutation bug still FAIL here
        d = float(np.abs(np.asarray(img, np.float64) - np.asarray(ref_img, np.float64)).max())
        assert d <= 1e-5, f"{label}: images differ by {d:.3g} -- more than a different libm expf can explain"
        pytest.xfail(f"{label}: images differ, and this host's libm expf is not glibc's x86-64 FMA build ({HOST_LIBM_MISMATCHES} sampled "
                     "disagreements with the restated algorithm): the bit-identity claim is 'glibc expf (FMA build) + uncontracted render.comp'")
    if not np.array_equal(a, b):
        bad = np.argwhere((a != b).any(axis=-1))
        d = np.abs(img.astype(np.float64) - ref_img).max()
        raise AssertionError(f"{label}: {len(bad)} pixel(s) differ in their bit patterns (max |d| {d:.3g}), first at (x, y) = "
                             f"({bad[0][1]}, {bad[0][0]})")


GUARD_TOL = 1e-5  # exp mode 3 against the reference text: rounding noise only (measured <= 4e-6), NO flip budget


def assert_guarded_close(rend, u, ref_img, label=""):
    """The frame of the library's DEFAULT blend (exp mode 3: v_exp_f32 under the guard of render.comp:82, every :78 decision
    taken on the alpha cut) against the reference text's frame: max abs <= GUARD_TOL on every pixel -- no threshold-flip
    budget, nothing to explain.  Returns (max abs, quadrants re-rendered with the reference's arithmetic, break decisions resolved
    by an exact per-pixel replay); leaves the renderer in exp mode 2."""
    rend.set_exp_mode(3)
    rend.set_blend_contraction(False)
    img, _ = rend.render_host(u)
    st = rend.stats()
    redo, resolved = st.blend_redo, st.blend_resolved
    rend.set_exp_mode(2)
    d = np.abs(img[..., :3].astype(np.float64) - ref_img[..., :3])
    worst = float(d.max()) if d.size else 0.0
    if not worst <= GUARD_TOL:
        ys, xs = np.nonzero(d.max(axis=2) > GUARD_TOL)
        raise AssertionError(f"{label}: guarded blend differs from the reference text by {worst:.3g} (> {GUARD_TOL}) at "
                             f"{len(ys)} pixel(s), first (x, y) = ({xs[0]}, {ys[0]})")
    assert (img[..., 3] == 1).all()
    return worst, int(redo), int(resolved)


def compare_images(img, ref_img, ref, width, label="", max_flips=None):
    """FAST-MODE comparison.  img vs ref_img (both H x W x >=3), lists taken from `ref` (attr, boundaries, sorted_payload).
    Asserts: every pixel differing by more than ULP_NOISE is an explained threshold flip (or within the cancellation bound
    of a contracted `power`), and there are at most max_flips of them: callers of the named configs pass the count observed
    for their case + 1; sweeps leave it None = max(3, 3 per 1e8 (pixel, entry) evaluations) (config B: 6 in 1.25e9).
    Returns (max diff over unflipped pixels, list of flipped pixels)."""
    d = np.abs(img[..., :3].astype(np.float64) - ref_img[..., :3]).max(axis=2)
    ys, xs = np.nonzero(d > ULP_NOISE)
    flips = []
    for py, px in zip(ys.tolist(), xs.tolist()):
        near = classify_pixel(ref["attr"], ref["boundaries"], ref["sorted_payload"], width, px, py)
        flipped = near["alpha"] < ALPHA_REL or near["T"] < T_REL or near["power"] < POWER_REL
        cancelled = d[py, px] <= CANCEL_SLACK * near["cancel"]   # contraction sensitivity of a cancelling `power`, no flip
        assert flipped or cancelled, (f"{label} pixel ({px},{py}) differs by {d[py, px]:.3g} with no entry near a threshold "
                                      f"and a cancellation bound of {near['cancel']:.3g}: {near}")
        if flipped and not cancelled:
            flips.append((px, py, float(d[py, px]), near))
    if max_flips is None:
        max_flips = max(3, int(3e-8 * 256.0 * len(ref["sorted_payload"])))
    assert len(flips) <= max_flips, f"{label}: {len(flips)} threshold-flip pixels (allowed {max_flips}): " \
                                    f"{[(x, y, round(dd, 6)) for x, y, dd, _ in flips]}"
    assert d.max() <= 2.0 / 255.0 * max(1.0, float(np.abs(ref_img[..., :3]).max()))
    rest = d.copy()
    rest[ys, xs] = 0
    return float(rest.max()), flips


# ---------------------------------------------------------------- the Python wrappers without a device
class FakeTensor:
    """The attributes the wrappers of binding.py read of a tensor, without torch or a device: what a device tensor of
    another framework would offer."""

    def __init__(self, shape, dtype="torch.float32", device="cuda:0", contiguous=True):
        self.shape, self.dtype, self._c = shape, dtype, contiguous

        class D:
            type, index = device.split(":")[0], (int(device.split(":")[1]) if ":" in device else None)
        self.device = D

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return self._c


class NoC:
    """In place of the C library: a wrapper that has checked its arguments and goes on to C raises this AssertionError."""

    def __getattr__(self, name):
        raise AssertionError("the C library was reached")


def forbid_c(pkg, monkeypatch):
    monkeypatch.setattr(pkg.binding, "lib", lambda: NoC())


def hand_made_scene(pkg, n=100):
    """A Scene of `n` Gaussians on device 0 that holds no handle: num_vertices does not ask C."""
    class SceneStub(pkg.Scene):
        num_vertices = n
    return SceneStub(None)


def hand_made_renderer(pkg, n=100, frame_hw=(40, 72), frames=1):
    """A Renderer that was never created in C: a scene of `n` Gaussians on device 0, `frame_hw` the last of `frames` frames."""
    rend = object.__new__(pkg.Renderer)
    rend.scene, rend._h, rend._frame_hw, rend._frames = hand_made_scene(pkg, n), None, frame_hw, frames
    return rend

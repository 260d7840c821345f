"""A seeded sweep over the last-frame passes and one step of a trainer, on the device: what tests/test_gpu_fuzz.py is to the
per-frame kernels.  Every case of tests/trainer_sweep_cases.py (24 drawn ones of up to 900 Gaussians on frames of 1 x 1 to
160 x 120, and WIDE: three of 3 000 Gaussians at 256 x 144, 144 tiles) goes through, in this order, each step against the
reference and the bound of that pass's own test file, whose guarded views, preloads and 8-byte-only alignment are imported, not
copied:

  1. the scene (from_records, or from_tensors of K < 15 coefficients; binary16 SH, a copy in spatial order where drawn) and the
     renderer with the drawn switches (antialiased, the one-pass level 1, the tile cull, the exp mode);
  2. the frame: the tiles tap and the image against the oracle -- bit for bit in exp mode 2, assert_guarded_close in mode 3; an
     antialiased frame is the plain frame of the scene S' that holds the frame's compensated opacities (the record tap).  Then the
     frame the passes read, queued behind two frames of other cameras where drawn, as launches or as replayed graphs;
  3. contributions and feature_maps (every output) bit for bit, lift_pixels under the drawn pixel mask within its bound;
  4. blend_backward, all four sums, with or without grad_alpha, within backward_reference.bound; rows without terms keep the
     preload's bits;
  5. project_backward at K and camera_backward on those sums within their bounds, each called a second time into the same arrays;
  6. visible_mask and densify_stats bit for bit;
  7. one Scene.adam_step of all six groups under the drawn Gaussian mask with the gradients of step 5: parameters, moments and the
     zeroed gradients bit for bit; a frame rendered after it is the frame of a fresh scene built from the stepped tensors;
  8. one densify of the stepped model under a rule whose thresholds are quantiles of the case's own statistic, bit for bit.

Nothing is left out of a comparison but the Gaussians trainer_sweep_cases.ill_conditioned names (none in these cases:
tests/test_trainer_sweep_cases.py).  A frame with no visible Gaussian is a case like any other: every output keeps its bits.

Each comparison against a bound prints its worst error / bound.  The largest seen per pass over the 27 cases on both depth-order
paths, on an MI355X:
    lift_pixels        0.222   (wide 1)
    blend_backward     0.0894  (conic, seed 18; colour 0.0737, opacity 0.0649, uv 0.0587)
    project_backward   0       (the first call into the preloaded pattern and the call into zeros: on every case the device's
                               sums are the reference's bit for bit); 0.5 after the second call into the same arrays (sh_dc and
                               sh_rest, seed 3; means 0.273, log_scales 0.4, quats 0.384, opacity_logits 0.4)
    camera_backward    0.00082 (the first call); 0.016 after the second (proj_mat, seed 14)
None is near 1.  The figures after a second call are those of the adds, not of the gradient: got = fl(fl(x + g) + g) against
x + 2 g, up to half an ulp of the content against a bound of 2 |content| 2^-53 -- a ratio of up to 0.5 whatever the kernel
computes.

Beside the sweep: the wait for the caller's queued work (binding._complete_callers_work) of the eight passes that had no test of
it -- blend_backward, project_backward, camera_backward, visible_mask, densify_stats, photometric_loss, Scene.adam_step, densify."""
import numpy as np
import pytest
import torch  # at collection, before the package loads its library: both must bind the same HIP runtime

import adam_step_reference as ar
import backward_cameras as bc
import backward_reference as bref
import contribution_reference as cref
import densify_reference as dr
import feature_reference as fref
import helpers
import lift_reference as lref
import project_backward_reference as pref
import test_gpu_adam_step as tas
import test_gpu_blend_backward as tbb
import test_gpu_camera_backward as tcb
import test_gpu_contributions as tco
import test_gpu_densify as tde
import test_gpu_feature_maps as tfm
import test_gpu_lift as tli
import test_gpu_project_backward as tpb
import trainer_sweep_cases as tsc
from test_adam_step_api import LR
from test_gpu_device_arrays import raw_blob, same

pytestmark = pytest.mark.gpu

SH_DEGREE = {0: 0, 3: 1, 8: 2, 15: 3}
OTHER_CAMERAS = ("C1", "C2")          # the two frames queued ahead of the case's where three are in flight
_cache = {}


def _frame(pkg, oracle, c):
    """(records, vertices, uniforms, the oracle's plain frame) of a case, on coefficients rounded to binary16 where the scene is read
    from that storage: computed once, never changed."""
    key = ("frame", c["name"])
    if key not in _cache:
        rec = tsc.records(pkg.synth, c)
        verts = oracle.activate_records(rec)
        if c["sh16"]:
            verts["sh"] = verts["sh"].astype(np.float16).astype(np.float32)
        u = oracle.camera_uniforms(tsc.camera(oracle, c), c["width"], c["height"])
        rec.setflags(write=False)
        _cache[key] = (rec, verts, u, oracle.stages(verts, u))
    return _cache[key]


def _frame_of_the_mode(oracle, rend, c, verts, u, plain):
    """(the oracle's frame the device's is compared with, what it was made from).  An antialiased frame is the plain frame of the
    scene whose opacities are the frame's compensated ones, read from the record tap: the contract tests/test_gpu_antialiased.py
    pins bit for bit."""
    if not c["antialiased"]:
        return plain, b""
    vis = plain["tiles"] != 0
    op = rend.stage("conic_opacity").reshape(-1, 4)[:, 3]
    assert (op[vis] <= verts["scale_opacity"][vis, 3]).all()
    key = ("prime", c["name"], op[vis].tobytes())
    if key not in _cache:
        prime = verts.copy()
        prime["scale_opacity"][vis, 3] = op[vis]
        _cache[key] = oracle.stages(prime, u)
    return _cache[key], op[vis].tobytes()


def _references(oracle, c, ref, tap):
    """The references that do not depend on what the device returned: contributions, feature maps, the lift and the blend's
    backward of the case's frame, with the case's seeded inputs.  Computed once per frame (both depth-order paths share them)."""
    key = ("references", c["name"], tap)
    if key not in _cache:
        n, w, h = c["n"], c["width"], c["height"]
        mask = tsc.pixel_mask(c)
        feats, vals = tfm._features(n, c["channels"], seed=11 + c["seed"]), tli._values(h, w, c["channels"], seed=23 + c["seed"])
        G, ga = tsc.grads(c)
        blend = bref.backward(oracle, ref, w, h, G, ga)
        del blend["pairs"]
        _cache[key] = dict(mask=mask, feats=feats, vals=vals, G=G, ga=ga, blend=blend, contributions=cref.contributions(oracle, ref, w, h, mask),
                           features=fref.feature_maps(oracle, ref, w, h, feats), lift=lref.lift(oracle, ref, w, h, vals, mask))
    return _cache[key]


def _scene(pkg, c, rec):
    if c["k"] < 15:
        gs = pkg.Scene.from_tensors(**{name: tas.device(a) for name, a in ar.cut(rec, c["k"]).items()})
    else:
        gs = pkg.Scene.from_records(rec, device=0)
    if c["sh16"]:
        gs.quantize_sh()
    return gs


def _renderer(pkg, gs, c):
    rend = pkg.Renderer(gs)
    rend.set_antialiased(c["antialiased"])
    if c["one_pass"]:
        rend.set_level1_fused(1)
    rend.set_tile_cull(c["tile_cull"])
    rend.set_exp_mode(c["exp_mode"])
    return rend


def _assert_frame(img, ref, c, label):
    if c["exp_mode"] == 2:
        helpers.assert_images_identical(img, ref["image"], label)
    else:
        d = np.abs(img[..., :3].astype(np.float64) - ref["image"][..., :3])
        assert (d <= helpers.GUARD_TOL).all() and (img[..., 3] == 1).all(), (label, float(d.max()))


def _queue_the_frame(pkg, rend, c, u):
    """The frame the passes read, as the case draws it: alone or behind two frames of other cameras, launched or replayed from
    captured graphs (the second round replays).  Returns the device tensors rendered into, the case's frame last."""
    w, h = c["width"], c["height"]
    rend.set_graph_mode(c["graph"])
    if c["in_flight"] == 3:
        rend.set_frames_in_flight(3)
    others = [pkg.camera_uniforms(bc.camera(pkg, cam), w, h) for cam in OTHER_CAMERAS] if c["in_flight"] == 3 else []
    targets = []                                               # (all kept: a frame in flight writes into its own)
    for _ in range(2 if c["graph"] else 1):
        targets += [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(len(others) + 1)]
        torch.cuda.synchronize()
        for uniforms, t in zip(others + [u], targets[-len(others) - 1:]):
            rend.render(uniforms, t.data_ptr(), 0)
    return targets


def _rule(pkg, params, h_stats):
    """Thresholds that are quantiles of the case's own statistic, as the end-to-end test of tests/test_gpu_densify.py takes them, so
    that some of each class clone, split and are pruned; the defaults where the frame saw no Gaussian."""
    seen = h_stats["count"] != 0
    if not seen.any():
        return dr.rule()
    q = dr.quantities(pkg, params, h_stats)
    return dr.rule(grad_threshold=float(np.quantile(q["avg"][seen], 0.6)), dense_extent=float(np.median(q["s"][seen])),
                   min_opacity=float(np.quantile(q["o"], 0.1)), max_screen_radius=float(np.quantile(q["radius"][seen], 0.95)))


@pytest.mark.parametrize("c", tsc.cases(), ids=lambda c: c["name"].replace(" ", "_"))
def test_a_drawn_case_through_every_last_frame_pass_and_one_step_of_a_trainer(pkg, oracle, gpu, _sort_path, monkeypatch, c):
    n, w, h, k, preload, name = c["n"], c["width"], c["height"], c["k"], c["preload"], c["name"]
    rec, verts, u_ref, plain = _frame(pkg, oracle, c)
    if c["spatial"]:
        monkeypatch.setenv("GS_SPATIAL_MIN", "1")              # the scene gets its copy in spatial order whatever its size
    else:
        monkeypatch.delenv("GS_SPATIAL_MIN", raising=False)
    # ---- 1. the scene and the renderer
    gs = _scene(pkg, c, rec)
    rend = _renderer(pkg, gs, c)
    closing = [rend, gs]
    try:
        u = pkg.camera_uniforms(tsc.camera(pkg, c), w, h)
        assert u.tobytes() == u_ref.tobytes()
        # ---- 2. the frame
        first, _ = rend.render_host(u)
        assert np.array_equal(rend.stage("tiles"), plain["tiles"]), f"{name}: the tiles tap"
        ref, tap = _frame_of_the_mode(oracle, rend, c, verts, u_ref, plain)
        assert np.array_equal(ref["tiles"], plain["tiles"])
        _assert_frame(first, ref, c, f"{name}: the frame")
        if c["exp_mode"] == 3:
            helpers.assert_guarded_close(rend, u, ref["image"], label=f"{name}: guarded blend")   # (leaves the renderer in mode 2)
            rend.set_exp_mode(3)
        targets = _queue_the_frame(pkg, rend, c, u)
        r = _references(oracle, c, ref, tap)
        visible = plain["tiles"] != 0
        print(f"{name}: {n} Gaussians at {w} x {h}, {int(visible.sum())} visible, {len(ref['keys'])} instances, lists culled: {rend.tile_cull()[1]}")
        # ---- 3. contributions, feature_maps, lift_pixels
        w0, p0 = (2 ** 32 - 1, 2 ** 31 - 1) if preload else (0, 0)
        out = tco.Arrays(n, h, w, weight0=w0, pixels0=p0)
        rend.contributions(mask=tco._mask_tensor(r["mask"]), **out.t)
        _assert_frame(targets[-1].cpu().numpy(), ref, c, f"{name}: the frame the passes read")        # (the first pass has drained the queue)
        assert np.array_equal(rend.stage("tiles"), plain["tiles"]), f"{name}: the tiles tap of the frame the passes read"
        tco._assert_equal(out, r["contributions"], f"{name} [contributions]", weight0=w0, pixels0=p0)
        tfm._run(rend, r["feats"], r["features"], h, w, f"{name} [feature_maps]")
        tli._run(rend, r["vals"], r["lift"], n, f"{name} [lift_pixels]", mask=r["mask"], preload=preload)
        # ---- 4. blend_backward
        G, ga, blend = r["G"], r["ga"], r["blend"]
        grad = (tli._offset_view(G, torch.float32, 1), None if ga is None else tli._offset_view(ga, torch.float32, 1))
        d = tbb.Sums(n, preload=preload)
        assert sorted(rend.blend_backward(*grad, **d.t)) == sorted(d.t)
        tbb._assert_close(d, blend, f"{name} [blend_backward]")
        if preload:                                            # from zeros: the sums the next passes take on
            d = tbb.Sums(n)
            rend.blend_backward(*grad, **d.t)
            tbb._assert_close(d, blend, f"{name} [blend_backward] from zeros")
        g = {key: d.get(key) for key in tpb.INS}
        uv = g["uv"].copy()
        # ---- 5. project_backward at K, camera_backward
        want = tpb._want(verts, u, ref, g, c["antialiased"], c["sh16"], k)
        ill = tsc.ill_conditioned(want) if c["antialiased"] else np.zeros(n, bool)
        skip = list(np.nonzero(ill)[0]) or None
        arr = tpb.Arrays(n, k)
        for times in (1, 2):
            got = rend.project_backward(**d.t, out=dict(arr.t))
            assert sorted(got) == sorted(arr.t)
            tpb._assert_close(arr, want, f"{name} [project_backward] call {times}", times=times, skip_rows=skip)
        d.guards_intact()
        d_cam = d.t
        if ill.any():                                          # such a Gaussian's share of a sum cannot be left out: its inputs are zeroed
            d_cam = {key: t.clone() for key, t in d.t.items()}
            for key in d_cam:
                d_cam[key][torch.as_tensor(ill).cuda()] = 0.0
                g[key][ill] = 0.0
        want_cam = tcb._want(verts, u, ref, g, c["antialiased"], c["sh16"])
        assert want_cam["n_visible"] == visible.sum()
        cam = tcb.Arrays(zeros=not preload)
        for times in (1, 2):
            assert sorted(rend.camera_backward(**d_cam, **cam.kwargs())) == sorted(tcb.NAMES)
            tcb._assert_close(cam, want_cam, f"{name} [camera_backward] call {times}", times=times)
        # ---- 6. visible_mask, densify_stats
        mask = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        assert rend.visible_mask(out=mask) is mask
        assert np.array_equal(mask.cpu().numpy(), visible.astype(np.uint8)), f"{name}: visible_mask"
        stats = pkg.densify_stats_zeros(gs)
        want_stats = dr.zero_stats(n)
        if preload:                                            # what an invisible row must keep
            stats["grad_sum"].fill_(0.5), stats["count"].fill_(3), stats["max_radius"].fill_(2.0)
            want_stats = dict(grad_sum=np.full(n, 0.5), count=np.full(n, 3, np.uint32), max_radius=np.full(n, 2.0, np.float32))
        assert rend.densify_stats(d.t["uv"], stats) is stats
        dr.accumulate_stats(want_stats, uv, plain["tiles"], ref["attr"]["color_radii"][:, 3], w, h)
        tas.same_bits(stats["grad_sum"], want_stats["grad_sum"], f"{name}: densify_stats: grad_sum")
        assert np.array_equal(stats["count"].cpu().numpy().view(np.uint32), want_stats["count"]), f"{name}: densify_stats: count"
        assert np.array_equal(stats["max_radius"].cpu().numpy(), want_stats["max_radius"]), f"{name}: densify_stats: max_radius"
        # ---- 7. one Adam step of the six groups with the gradients of this frame, as the wrapper allocates them
        fresh = rend.project_backward(**d.t, sh_degree=SH_DEGREE[k])
        for key in tpb.NAMES:
            assert tuple(fresh[key].shape) == want[key].shape, key
            err, lim = np.abs(fresh[key].cpu().numpy() - want[key])[~ill], pref.bound(want, key)[~ill]
            print(f"{name} [project_backward_into_zeros]: {key}: worst error / bound = {float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0:.3g}")
            assert (err <= lim).all(), f"{name}: project_backward into the wrapper's zeros: {key}"
        rend.synchronize()
        run = tas.Run(pkg, rec, k, scene=gs, lr={key: 20 * v for key, v in LR.items()})
        run.step(tsc.gaussian_mask(c), grads={key: fresh[key].cpu().numpy() for key in run.host})
        run.check_tensors(f"{name}: adam_step")
        after, _ = rend.render_host(u)
        fresh_scene = run.fresh_scene()
        closing.append(fresh_scene)
        if c["sh16"]:
            fresh_scene.quantize_sh()
        fresh_rend = _renderer(pkg, fresh_scene, c)
        closing.insert(0, fresh_rend)
        want_after, _ = fresh_rend.render_host(u)
        same(gs.download_vertices(), fresh_scene.download_vertices(), f"{name}: vertices after the step")
        same(raw_blob(gs), raw_blob(fresh_scene), f"{name}: the blob after the step")
        assert np.array_equal(rend.stage("tiles"), fresh_rend.stage("tiles")), f"{name}: the tiles tap after the step"
        assert np.array_equal(after.view(np.uint32), want_after.view(np.uint32)), f"{name}: the frame after the step"
        # ---- 8. one densify of the stepped model
        h_stats = {key: t.cpu().numpy() for key, t in stats.items()}
        h_stats["count"] = h_stats["count"].view(np.uint32)
        noise = np.random.default_rng(6000 + c["seed"]).standard_normal((n, 2, 3)).astype(np.float32)
        model = dict(params={key: a.copy() for key, a in run.host.items()}, moments=dict(exp_avg=run.m, exp_avg_sq=run.v), stats=h_stats,
                     rule=_rule(pkg, run.host, h_stats), noise=noise)
        p, _ = tde.check(pkg, model, f"{name}: densify")
        print(f"{name}: densify: {n} -> {p['n_out']} rows, {p['n_noise']} parents split")
    finally:
        for handle in closing:
            handle.close()


# ------------------------------------------------------------------------------------------------ the caller's queued work
class Feed:
    """Device tensors of a call.  queued: each is made holding something else (NaN; an integer with its lowest bit flipped), and
    release() queues milliseconds of elementwise work on torch's current stream (the filler of tests/test_gpu_lift.py) and, behind
    it, the copies that give every tensor its contents -- the inputs' fill and the outputs' zeroing, still running when the pass
    is called.  Not queued: the contents are in place and the device idle before the call."""

    def __init__(self, queued):
        self.queued, self.late, self.keep = queued, [], None

    def __call__(self, final):
        final = (final if torch.is_tensor(final) else torch.as_tensor(np.ascontiguousarray(final))).cuda()
        if not self.queued:
            return final.clone()
        t = torch.full_like(final, float("nan")) if final.is_floating_point() else final.bitwise_xor(1)
        self.late.append((t, final))
        return t

    def release(self):
        torch.cuda.synchronize()
        if self.queued:
            self.keep = tli._queue_filler()
            for t, final in self.late:
                t.copy_(final)


@pytest.fixture(scope="module")
def frame_a(pkg, oracle, gpu):
    """Scene A of tests/test_gpu_blend_backward.py, rendered; the blend's reference; the sums of one blend_backward made with the
    device idle; a second stream of torch's for the two calls that run on the caller's."""
    kind = "A"
    n, w, h = tbb.SCENES[kind]
    ref, G, ga, want = tbb._reference(pkg, oracle, kind)
    gs, rend = tbb._open(pkg, kind)
    rend.render_host(tbb._uniforms(pkg, kind))
    torch.cuda.synchronize()
    d = rend.blend_backward(torch.as_tensor(G).cuda(), torch.as_tensor(ga).cuda(), colour=True, opacity=True, conic=True, uv=True)
    ctx = dict(pkg=pkg, rend=rend, n=n, w=w, h=h, G=G, ga=ga, blend=want, visible=ref["tiles"] != 0, side=torch.cuda.Stream(),
               sums={name: t.cpu().numpy() for name, t in d.items()}, rec=pkg.synth.synth_records(n, seed=5, kind=kind))
    yield ctx
    rend.close()
    gs.close()


def _host(tensors):
    return {name: t.cpu().numpy() for name, t in tensors.items()}


def _queued_blend_backward(x, feed):
    G, ga = feed(x["G"]), feed(x["ga"])
    out = {name: feed(np.zeros(shape)) for name, shape in x["pkg"].binding._record_shapes(x["n"]).items()}
    feed.release()
    x["rend"].blend_backward(G, ga, **out)
    return _host(out)


def _queued_project_backward(x, feed):
    sums = {name: feed(a) for name, a in x["sums"].items()}
    out = {name: feed(np.zeros(shape)) for name, shape in tpb._shapes(x["n"], 15).items()}
    feed.release()
    x["rend"].project_backward(**sums, out=out)
    return _host(out)


def _queued_camera_backward(x, feed):
    sums = {name: feed(a) for name, a in x["sums"].items()}
    out = dict(view_mat=feed(np.zeros(16)), proj_mat=feed(np.zeros(16)), camera_position=feed(np.zeros(3)))
    feed.release()
    x["rend"].camera_backward(**sums, **out)
    return _host(out)


def _queued_visible_mask(x, feed):
    out = feed(np.zeros(x["n"], np.uint8))
    feed.release()
    x["rend"].visible_mask(out=out, accumulate=True)          # (ORed into zeros that a late fill must not wipe)
    got = out.cpu().numpy()
    assert np.array_equal(got, x["visible"].astype(np.uint8))
    return dict(mask=got)


def _queued_densify_stats(x, feed):
    n = x["n"]
    uv = feed(x["sums"]["uv"])
    stats = dict(grad_sum=feed(np.zeros(n)), count=feed(np.zeros(n, np.int32)), max_radius=feed(np.zeros(n, np.float32)))
    feed.release()
    x["rend"].densify_stats(uv, stats)
    return _host(stats)


def _queued_photometric_loss(x, feed):
    rng = np.random.default_rng(12)
    image, target = (feed(rng.random((x["h"], x["w"], 3)).astype(np.float32)) for _ in range(2))
    grad, terms = feed(np.zeros((x["h"], x["w"], 3), np.float32)), feed(np.zeros(4))
    feed.release()
    x["rend"].photometric_loss(image, target, 0.2, grad=grad, terms=terms)
    return dict(grad=grad.cpu().numpy(), terms=terms.cpu().numpy())


def _queued_adam_step(x, feed):
    """On a scene of its own (the step changes it), on a second stream of torch's: Scene.adam_step waits for torch's CURRENT
    stream, where its tensors are still being written, whatever stream it runs on."""
    pkg, n = x["pkg"], x["n"]
    host = ar.cut(x["rec"])
    scene = pkg.Scene.from_tensors(**{name: tas.device(a) for name, a in host.items()})
    try:
        params = {name: feed(a) for name, a in host.items()}
        grads = {name: feed(g) for name, g in ar.random_gradients(host, seed=51).items()}
        m, v = ({name: feed(np.zeros(a.shape, np.float32)) for name, a in host.items()} for _ in range(2))
        mask = feed((np.arange(n) % 3 != 0).astype(np.uint8))
        feed.release()
        scene.adam_step(params, grads, m, v, LR, ar.BETAS, ar.EPS, 1, mask=mask, stream=x["side"])
        out = {f"{what} of {name}": t.cpu().numpy() for what, d in dict(param=params, grad=grads, exp_avg=m, exp_avg_sq=v).items() for name, t in d.items()}
        return dict(out, vertices=scene.download_vertices())
    finally:
        scene.close()


def _queued_densify(x, feed):
    pkg, n = x["pkg"], 300
    sc = dr.scene(pkg, n, seed=2, k=3)
    params = {name: feed(a) for name, a in sc["params"].items()}
    state = {what: {name: feed(a) for name, a in sc["moments"][what].items()} for what in ("exp_avg", "exp_avg_sq")}
    stats = dict(grad_sum=feed(sc["stats"]["grad_sum"]), count=feed(sc["stats"]["count"].view(np.int32)), max_radius=feed(sc["stats"]["max_radius"]))
    noise = feed(sc["noise"])
    feed.release()
    new, new_state, info = pkg.densify(tde.Model(n), params, sc["rule"], stats, state, noise=noise, stream=x["side"])
    assert 0 < info["n_noise"] and n // 2 < info["n_out"]
    out = {f"{what} of {name}": t.cpu().numpy() for what, d in dict(param=new, **new_state).items() for name, t in d.items()}
    return dict(out, row_offset=info["row_offset"].cpu().numpy(), noise_offset=info["noise_offset"].cpu().numpy())


QUEUED = dict(blend_backward=_queued_blend_backward, project_backward=_queued_project_backward, camera_backward=_queued_camera_backward,
              visible_mask=_queued_visible_mask, densify_stats=_queued_densify_stats, photometric_loss=_queued_photometric_loss,
              adam_step=_queued_adam_step, densify=_queued_densify)


@pytest.mark.parametrize("which", list(QUEUED))
def test_inputs_and_zeroed_outputs_still_queued_on_torchs_stream_are_complete_before_the_pass(frame_a, which):
    """The passes over the last frame run on the renderer's own non-blocking stream, Scene.adam_step and densify on whatever stream
    they are given: none is ordered behind torch's current stream by anything but the wait the wrapper makes first
    (binding._complete_callers_work).  Here every input's fill and every output's zeroing is queued on torch's stream behind
    several milliseconds of other work immediately before the call; the result is that of the same call made with the device
    idle -- bit for bit where the pass is deterministic, within the bound of its definition for blend_backward's atomic sums.
    Without the wait the pass reads NaNs, or its sums are wiped by the late fill."""
    calm, busy = (QUEUED[which](frame_a, Feed(queued)) for queued in (False, True))
    assert sorted(calm) == sorted(busy)
    for name, want in calm.items():
        got = busy[name]
        assert got.shape == want.shape and got.dtype == want.dtype, (which, name)
        assert want.size == 0 or want.any(), f"{which}: {name} is all zero: the comparison would not notice a wiped output"
        if which == "blend_backward":
            for a in (want, got):
                assert (np.abs(a - frame_a["blend"][name]) <= bref.bound(frame_a["blend"], name)).all(), f"{which}: {name}"
        else:
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{which}: {name} differs from the call made with the device idle"

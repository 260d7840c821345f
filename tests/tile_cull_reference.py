"""What the tile-cull tests share: the rule of 3dgs.cpp_amd/csrc/gs_tile_cull.h compiled for the CPU, and the property a dropped
(tile, Gaussian) must have -- no pixel of the tile passes render.comp:68/:78 with `power` evaluated in binary32 as the shader
writes it (:66: every product and sum rounded, no contraction) and :78 taken on the Gaussian's alpha cut (oracle.alpha_cut)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dgs.cpp_amd", "csrc")
TILE = 16


def build_rule(out_dir):
    out = os.path.join(str(out_dir), "libtile_cull_sim.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "tile_cull_sim.cpp"), "-o", out])
    return C.CDLL(out)


def tight_boxes(lib, conic, uv, cut, ref):
    """conic [n, 3], uv [n, 2], cut [n], ref [n, 4] tile boxes (upper bounds exclusive) -> tight [n, 4] (all zero: empty)."""
    conic = np.ascontiguousarray(conic, np.float32)
    uv = np.ascontiguousarray(uv, np.float32)
    cut = np.ascontiguousarray(cut, np.float32)
    ref = np.ascontiguousarray(ref, np.int32)
    out = np.zeros_like(ref)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib.tc_boxes(p(conic), p(uv), p(cut), p(ref), C.c_uint64(len(ref)), p(out))
    return out


def frame_inputs(oracle, attr, tiles):
    """(ids of the visible Gaussians, conic, uv, cut, reference boxes) of a frame's oracle.preprocess output."""
    ids = np.nonzero(tiles)[0]
    co = attr["conic_opacity"][ids]
    return ids, co[:, :3], attr["uv"][ids], oracle.alpha_cut(co[:, 3]), attr["aabb"][ids].astype(np.int32)


def assert_contained(ref, tight):
    empty = (tight == 0).all(axis=1)
    inside = (tight[:, 0] >= ref[:, 0]) & (tight[:, 1] >= ref[:, 1]) & (tight[:, 2] <= ref[:, 2]) & (tight[:, 3] <= ref[:, 3]) & \
             (tight[:, 0] < tight[:, 2]) & (tight[:, 1] < tight[:, 3])
    assert (empty | inside).all(), np.nonzero(~(empty | inside))[0][:8]


def kept_instances(box):
    return int(((box[:, 2] - box[:, 0]).astype(np.int64) * (box[:, 3] - box[:, 1])).sum())


def shader_power(a, b, c, u, v, px, py):
    """render.comp:66 in binary32, one rounding per operation, in the order written."""
    f = np.float32
    dx, dy = (u - px.astype(f)).astype(f), (v - py.astype(f)).astype(f)
    t = ((a * dx).astype(f) * dx).astype(f) + ((c * dy).astype(f) * dy).astype(f)
    return (f(-0.5) * t.astype(f)).astype(f) - ((b * dx).astype(f) * dy).astype(f)


def dropped_tiles(ref, tight):
    """(index into the arrays, tile x, tile y) of every tile of a reference box outside its tight box."""
    gi, tx, ty = [], [], []
    for i in np.nonzero(((ref[:, 2] - ref[:, 0]) * (ref[:, 3] - ref[:, 1])) != kept_per_box(tight))[0]:
        xs, ys = np.meshgrid(np.arange(ref[i, 0], ref[i, 2]), np.arange(ref[i, 1], ref[i, 3]))
        out = ~((xs >= tight[i, 0]) & (xs < tight[i, 2]) & (ys >= tight[i, 1]) & (ys < tight[i, 3]))
        gi.append(np.full(int(out.sum()), i))
        tx.append(xs[out])
        ty.append(ys[out])
    if not gi:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(gi), np.concatenate(tx), np.concatenate(ty)


def kept_per_box(box):
    return (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])


def assert_dropped_pairs_unused(conic, uv, cut, gi, tx, ty, chunk=1 << 14):
    """Every (Gaussian gi[k], tile (tx[k], ty[k])): none of the tile's 256 pixels has cut <= power <= 0.  Returns the pairs checked."""
    conic, uv, cut = np.asarray(conic, np.float32), np.asarray(uv, np.float32), np.asarray(cut, np.float32)
    ox, oy = np.meshgrid(np.arange(TILE), np.arange(TILE))
    ox, oy = ox.ravel()[None, :], oy.ravel()[None, :]
    for s in range(0, len(gi), chunk):
        g = gi[s:s + chunk]
        px, py = tx[s:s + chunk, None] * TILE + ox, ty[s:s + chunk, None] * TILE + oy
        p = shader_power(conic[g, 0, None], conic[g, 1, None], conic[g, 2, None], uv[g, 0, None], uv[g, 1, None], px, py)
        used = (p <= 0) & ~(p < cut[g, None])  # :68 keeps power <= 0; :78 keeps !(power < cut); a NaN power skips the entry
        if used.any():
            k, j = np.argwhere(used)[0]
            raise AssertionError(f"Gaussian index {g[k]} tile ({tx[s + k]}, {ty[s + k]}) was dropped but pixel ({px[k, j]}, {py[k, j]}) "
                                 f"keeps it: power {p[k, j]!r} cut {cut[g[k]]!r}")
    return len(gi)

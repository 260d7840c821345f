"""Scenes that stand exactly on a capacity or a cooperative step of the per-frame kernels.
  * binning and blend: the candidates a depth-order level holds, the run of equal depths the tie step orders in place, the keys a
    depth bucket holds before the stable passes take over, the slab cut, the items of a level-1 block, the bin box the whole
    wave emits, the blend's chunks of 64, the guard's list, replays and pairs;
  * k_bin_build (bins of 16 x 16 and 32 x 32 tiles, and every bin size of the global path): its one capacity of 16384, the
    sort rounds of 1024, a wave's run of the list, one tile that takes every candidate, boxes clipped to the bin, a bin cut
    by the frame's edge (build_size, build_unrefinable, build_one_tile, build_boxes, equal_run with shift 4 and 5);
  * k_preprocess (wave_patterns): every count of visible lanes of a wave at which the LDS-DMA fetch of the SH blocks, the wave's
    run of slots in the dense lists or the four-lanes-per-record store changes shape, in the lowest lanes, the highest, and
    spread; every exit of a culled lane; a ragged last wave; in index order and in a spatial order that is a known scramble of
    the ids (morton_order restates gs_host_math.h's spatial_order); and the dense lists full to their last slot (dense_lists_full);
  * the global depth order (radix_blocks): every shape of the radix passes' grid -- 1 to 4 entries per thread of the scan, a
    block that owns two tiles, later passes over V << N keys with a tile one key short, full and one over -- with depth
    patterns of extreme low bytes and equal depths across tiles and blocks.

Nothing here is random but the SH coefficients of the wave patterns (a fixed seed).  Every candidate is ONE tiny isotropic
Gaussian (radius 3 px) whose centre lies within 2.5 px of a tile's centre, so its tile box is that tile and nothing else; the
camera is the identity, so view depth is -z bit for bit and a scene's depths are written as binary32 bit patterns.  A builder
returns a LimitScene: the records, the frame, the environment the renderer needs, and `expect` -- the quantities it pins, exact by
construction.  The second half of the module re-measures those quantities from the oracle's stages (tests/test_limit_scenes.py
asserts they are equal, with no GPU) and restates the level policy of gs_depth_policy.h for a fresh renderer, which is where the
GPU test's predicted stats come from.  The last part restates what the one-pass level 1 (gs_kernels.h: L1Fused) depends on: the
default capacity of the candidate buffer, the region of it a bin owns, and which of these scenes run on that path.

A plain module: numpy and tests/ only."""
from dataclasses import dataclass, field

import numpy as np

from float64_cases import RECORD_FLOATS, _ndc, _place

FOV = 45.0
LEVEL_LIMITS = (4096, 8192, 12288, 16384, 65535)   # gs_levels.h: kBinSortLimit
SLAB_LEVEL, GLOBAL_LEVEL = 4, 5
SLAB_MAX = 12288                                    # candidates of one depth slab (gs_bin_l2.hip: MAXC of k_bin_slabs)
MAX_SLABS = 16                                      # kMaxSlabs
MSD_BUCKETS, MSD_BUCKET_MAX = 4096, 64              # kMsdBuckets, kMsdBucketMax
TIE_RUN_MAX = 65                                    # the longest run of equal depths the tie step orders in place
THREADS = 1024                                      # of a level-2 workgroup: element e of the ordered list is round e / 1024
BUILD_MAX = 16384                                   # gs_bin_l2.hip: MAXC of k_bin_build<R2, 1024, true>, at EVERY bin-local level
ONE_SIZE_SHIFT = 4                                  # gs_depth_policy.h: kOneSizeShift, the bins k_bin_build orders (no slabs)
L1_ITEMS, L1_XCD_RUN, L1_BIG_BOX = 1024, 32, 12     # gs_bin.h
BLEND_CHUNK = 64
WAVE, PRE_BLOCK = 64, 256                           # gs_device.h: a wave, a workgroup of k_preprocess (four waves)
VIS_REGIONS = 256                                   # gs_kernels.h: kVisRegions, the dense lists of visible Gaussians
SORT_TILE, SORT_MAX_BLOCKS, SCAN_THREADS = 2048, 1024, 256   # gs_kernels.h: kSortTileKeys, kSortMaxBlocks; k_radix_scan's workgroup
DEPTH_2 = 0x40000000                                # the bit pattern of 2.0f: [2, 4) holds 2^23 patterns
PRIME = 1000003


@dataclass
class LimitScene:
    name: str
    records: np.ndarray
    width: int
    height: int
    env: dict                      # environment of the renderer (GS_BIN_SHIFT, GS_L1_DENSE_MIN, ...)
    pins: str                      # the limit this scene stands on
    expect: dict                   # the pinned quantities, exact by construction (see measure())
    slabs_fail: bool = False       # the depth slabs cannot order the fullest bin (a long run, too many slabs)
    guard: dict = None             # guard scenes: the sites, the tuned layers, the quadrant, what the counters must say
    min_shift: int = field(init=False)

    def __post_init__(self):
        self.min_shift = int(self.env.get("GS_BIN_SHIFT", 3))


# ------------------------------------------------------------------------------------------------ placing
def _splats(depth_bits, tile_x, tile_y, w, h, logit=None, pixel=None):
    """One tiny Gaussian per entry, in id order: view depth = the binary32 pattern, tile box = exactly (tile_x, tile_y).
    pixel = (px, py): centred on those pixels instead (tile_x, tile_y unused)."""
    depth_bits = np.asarray(depth_bits, np.uint32)
    n = len(depth_bits)
    i = np.arange(n, dtype=np.int64)
    tz = depth_bits.view(np.float32)
    ux = 16.0 * np.asarray(tile_x, np.float64) + 7.5 + ((i * 7) % 5 - 2)
    uy = 16.0 * np.asarray(tile_y, np.float64) + 7.5 + ((i * 3) % 5 - 2)
    if pixel is not None:
        ux, uy = np.asarray(pixel[0], np.float64), np.asarray(pixel[1], np.float64)
    rec = np.zeros((n, RECORD_FLOATS), np.float32)
    _place(rec, _ndc(ux, w), _ndc(uy, h), tz.astype(np.float64), FOV, w, h)
    rec[:, 2] = -tz
    rec[:, 6] = np.sin(0.37 * i) * 1.2
    rec[:, 7] = np.cos(0.91 * i) * 1.2
    rec[:, 8] = np.sin(1.73 * i + 1.0) * 1.2
    rec[:, 54] = (-1.0 + 2.0 * ((i * 0.6180339887) % 1.0)) if logit is None else logit
    rec[:, 55:58] = np.log(tz.astype(np.float64) * 1e-5)[:, None]   # 0.01 px: the 0.3 px dilation is all of the footprint
    rec[:, 58] = 1.0
    return rec


def _bin_tiles(count, shift, bin_x, bin_y, first=0):
    """Tiles of bin (bin_x, bin_y) for `count` candidates, dealt round robin over the bin's S x S tiles."""
    s = 1 << shift
    k = (np.arange(count, dtype=np.int64) + first) % (s * s)
    return bin_x * s + k % s, bin_y * s + k // s


def _spread_bits(count, lo=DEPTH_2, span=1 << 23):
    """`count` distinct depth patterns in [lo, lo + span), scrambled against the id order."""
    stride = span // count
    assert stride >= 1
    return (lo + ((np.arange(count, dtype=np.int64) * PRIME) % count) * stride).astype(np.uint32)


def _background(shift, bins, skip, per_bin, w, h):
    """A few hundred splats in every other bin of the frame, so that the fullest bin is not the only one."""
    recs = []
    for by in range(bins[1]):
        for bx in range(bins[0]):
            if (bx, by) == skip or per_bin == 0:
                continue
            tx, ty = _bin_tiles(per_bin, shift, bx, by)
            recs.append(_splats(_spread_bits(per_bin, DEPTH_2 + 12345 * (1 + bx + 2 * by)), tx, ty, w, h))
    return np.concatenate(recs) if recs else np.zeros((0, RECORD_FLOATS), np.float32)


def _one_bin_scene(name, bits, shift, pins, expect, env=None, slabs_fail=False, frame_bins=2, first_tile=0, background=200,
                   tile=None):
    """`bits` (id order) all in bin (1, 1) of a frame of frame_bins x frame_bins bins of 2^shift tiles, dealt round robin over
    its tiles (or all in `tile`); `background` (200) in every other bin."""
    w = h = 16 * (1 << shift) * frame_bins
    bg = _background(shift, (frame_bins, frame_bins), (1, 1), background, w, h)
    tx, ty = _bin_tiles(len(bits), shift, 1, 1, first_tile)
    if tile is not None:
        tx, ty = np.full(len(bits), tile[0]), np.full(len(bits), tile[1])
    rec = np.concatenate([bg, _splats(bits, tx, ty, w, h)])
    e = dict(n=len(rec), visible=len(rec), fullest_bin={shift: len(bits)}, bin_entries={shift: len(rec)})
    e.update(expect)
    full_env = {"GS_BIN_SHIFT": str(shift)}
    full_env.update(env or {})
    return LimitScene(name, rec, w, h, full_env, pins, e, slabs_fail)


# ------------------------------------------------------------------------------------------------ level-2 sizes
def level2_size(count, shift=2):
    """The fullest bin holds exactly `count` candidates of distinct depths.  shift 2: bins of 4 x 4 tiles, which the policy
    cannot refine; shift 3 (the default): a frame whose bins can be halved, with the candidates dealt evenly over the bin's 64
    tiles, so that each of the four smaller bins holds a quarter of them."""
    sc = _one_bin_scene(f"level2_size/{count}@{shift}", _spread_bits(count), shift,
                        f"candidates in the fullest bin = {count}", {})
    if shift == 3:
        tx, ty = _bin_tiles(count, 3, 1, 1)
        quarter = np.bincount(((ty >> 2) & 1) * 2 + ((tx >> 2) & 1), minlength=4)
        sc.expect["fullest_bin"][2] = int(quarter.max())
        sc.expect["bin_entries"][2] = sc.expect["n"]
        del sc.env["GS_BIN_SHIFT"]
        sc.min_shift = 3
    return sc


# ------------------------------------------------------------------------------------------------ equal-depth runs
RUN_PLACES = ("start", "end", "straddle", "scattered")


def equal_run(length, place, slab, shift=2):
    """A bin of M distinct depths, one of which is shared by `length` Gaussians.  place: the run is the nearest of the bin
    ("start": ordered position 0), the farthest ("end"), begins 30 elements short of the ordered list's element 1024
    ("straddle": it crosses from one round of the workgroup to the next), or sits mid-bin with its ids scattered over the
    whole id range.  slab: 20 000 candidates (depth slabs, level 4) instead of 3 000 (k_bin_fast<4>).
    shift 4 or 5 (k_bin_build, which has no tie step and no tie limit: its four passes are stable and its input is in id
    order): the bin holds 3000 candidates IN ALL, the run among them, so that the workgroup takes ceil(3000 / 1024) = 3 rounds
    and wave w owns elements 192 w .. 192 w + 191 of the list; "straddle" begins 30 elements short of element 192 -- or, a run
    shorter than that, on element 191 -- and crosses from wave 0's elements into wave 1's."""
    m = 20000 if slab else 3000
    straddle = THREADS - 30
    if shift >= ONE_SIZE_SHIFT:
        assert not slab
        m -= length - 1
        straddle = 3 * WAVE - min(30, length - 1)
    rank = {"start": 0, "end": m - 1, "straddle": straddle, "scattered": m // 2 + 7}[place]
    ranks = (np.arange(m, dtype=np.int64) * PRIME) % m          # a permutation: rank of id j
    at = int(np.nonzero(ranks == rank)[0][0])
    extra = length - 1
    if place == "scattered":
        where = np.sort(((np.arange(extra, dtype=np.int64) * 7919 + 13) * (m // max(extra, 1))) % m)
    else:
        where = np.full(extra, at + 1)
    ranks = np.insert(ranks, where, rank)
    bits = (DEPTH_2 + ranks * ((1 << 23) // m)).astype(np.uint32)
    fails = slab and length > TIE_RUN_MAX
    return _one_bin_scene(f"equal_run/{length}/{place}/{'slab' if slab else 'fast' if shift < ONE_SIZE_SHIFT else shift}", bits, shift,
                          f"run of {length} equal depths at ordered position {rank}",
                          dict(longest_run=length, run_start=rank), slabs_fail=fails)


# ------------------------------------------------------------------------------------------------ k_bin_build
BUILD_COUNTS = (1, 64, 65, 1023, 1024, 1025, 16383, 16384)
BUILD_GLOBAL_COUNTS = (1, 1023, 1024, 1025, 16385)
BUILD_STREAMED = 70000


def build_size(count, shift):
    """k_bin_build's fullest bin holds exactly `count` candidates of distinct, scrambled depths, dealt round robin over the tiles
    of bin (1, 1) of a frame of 2 x 2 bins of 2^shift tiles (GS_BIN_SHIFT: 512 x 512 at shift 4, 1024 x 1024 at shift 5; shift
    3, 256 x 256, for the global path's k_bin_build<1, false>).  The other bins hold min(200, count - 1).
    k_bin_build<R2, 1024, true> holds 16384 candidates AT LEVEL 0 and at every other bin-local level -- its capacity is not
    sized by the level -- so every count up to 16384 stays at level 0 without a re-run (predict says the same).  16385 on
    these frames: the bins can be halved, and the policy does that first (shift 4 -> 3 and k_bin_fast<16>, 5 -> 4), each of
    the four smaller bins then holding a quarter."""
    sc = _one_bin_scene(f"build_size/{count}@{shift}", _spread_bits(count), shift,
                        f"candidates in the fullest bin of 2^{shift} tiles = {count}", {}, background=min(200, count - 1))
    if count > BUILD_MAX and shift >= ONE_SIZE_SHIFT:
        half = shift - 1
        tx, ty = _bin_tiles(count, shift, 1, 1)
        quarter = np.bincount(((ty >> half) & 1) * 2 + ((tx >> half) & 1), minlength=4)
        sc.expect["fullest_bin"][half] = int(quarter.max())
        sc.expect["bin_entries"][half] = sc.expect["n"]
    return sc


UNREFINABLE_FRAME = (4112, 256)                     # 257 x 16 tiles: bins of 16 x 16 tiles, 17 x 1 of them, and 33 x 2 of 8 x 8 do not fit


def build_unrefinable(count):
    """A frame that runs with bins of 16 x 16 tiles by itself (257 tiles across: no GS_BIN_SHIFT) and whose bins cannot be
    halved: 17 x 1 bins, the last of them ONE tile wide (the partial bin: 16 real tiles of its 256 slots).  Bin 1 holds `count`
    candidates, the one-tile-wide bin 16 holds 300 over its 16 tiles, every other bin 200."""
    w, h = UNREFINABLE_FRAME
    shift = 4
    recs = []
    for bx in range(17):
        k = count if bx == 1 else 300 if bx == 16 else 200
        tx, ty = _bin_tiles(k, shift, bx, 0)
        if bx == 16:
            j = np.arange(k, dtype=np.int64)
            tx, ty = np.full(k, 256), j % 16
        recs.append(_splats(_spread_bits(k, DEPTH_2 + 12345 * bx), tx, ty, w, h))
    rec = np.concatenate(recs)
    n = len(rec)
    return LimitScene(f"build_unrefinable/{count}", rec, w, h, {}, f"{count} candidates in a bin of 16 x 16 tiles that cannot be halved",
                      dict(n=n, visible=n, fullest_bin={shift: count}, bin_entries={shift: n},
                           bin_counts={shift: {(1, 0): count, (16, 0): 300}}, tile_columns_of_the_last_bin=1))


def build_one_tile(shift):
    """16384 candidates, all of them in ONE tile of the bin: every chunk of the fill adds 64 to that tile's 16-bit count of the
    round, every round moves its cursor by 1024, and the tile's list is 16384 long."""
    s = 1 << shift
    tile = (s + 5, s + 3)
    return _one_bin_scene(f"build_one_tile@{shift}", _spread_bits(BUILD_MAX), shift, f"a tile list of {BUILD_MAX} from one bin of 2^{shift} tiles",
                          dict(longest_tile_list=(tile, BUILD_MAX)), tile=tile)


BOX_PROBES = ("whole_bin", "tile_row", "tile_column", "four_bins", "frame_edge")
_BOX_PROBE_LANES = (5, 64 + 63, 200, 201, 3 * 64)  # of the bin's candidates, in id order: big_box's


def _probe(one, ux, uy, tz, radius, w, h):
    """Turn record `one` into a faint isotropic Gaussian centred on pixel (ux, uy) -- on the frame or off it -- whose radius is
    exactly `radius`.  radius = ceil(3 sqrt(lambda)); with v = the (clamped) view-space slopes of the centre, the projected
    covariance is s^2 (I + v v^T) + 0.3 I, so lambda = mid + sqrt(max(0.1, mid^2 - det)) with mid = s^2 (1 + |v|^2 / 2) + 0.3
    and mid^2 - det = (s^2 |v|^2 / 2)^2."""
    assert w == h
    tan = np.tan(np.radians(FOV) / 2.0)
    focal = w / (2.0 * tan)
    nx, ny = _ndc(np.array([ux], np.float64), w), _ndc(np.array([uy], np.float64), h)
    _place(one, nx, ny, np.array([tz]), FOV, w, h)
    one[:, 2] = -np.float32(tz)
    v2 = float((np.clip(nx * tan, -1.3 * tan, 1.3 * tan) ** 2 + np.clip(ny * tan, -1.3 * tan, 1.3 * tan) ** 2)[0])
    lam = (radius - 0.5) ** 2 / 9.0
    s2 = (lam - 0.3) / (1.0 + v2)
    if s2 * v2 / 2.0 < np.sqrt(0.1):
        s2 = (lam - 0.3 - np.sqrt(0.1)) / (1.0 + v2 / 2.0)
        assert s2 * v2 / 2.0 < np.sqrt(0.1)
    one[:, 55:58] = np.log(np.sqrt(s2) * tz / focal)
    one[:, 54] = -4.0


def build_boxes(shift):
    """Bin (1, 1) of 2 x 2 bins of S x S tiles holds 2995 single-tile candidates and five faint probes (3000: three rounds), placed
    like big_box's in lanes 5 and 63 of two waves, two neighbours and lane 0.  A tile box is a square around the centre, clamped
    to the frame; the bin is the frame's lower right quarter, so a probe centred beyond the frame's edge covers ONE row or column:
      whole_bin:    the S x S tiles of the bin and no other;
      tile_row:     the bin's last tile row, all S tiles of it (centred below the frame);
      tile_column:  the bin's last tile column (centred right of the frame);
      four_bins:    6 x 6 tiles around the corner the four bins share: 3 x 3 in each, clipped at another pair of edges in each;
      frame_edge:   4 x 6 tiles against the frame's right edge (the box would go on for two more columns).
    Every box edge that is not the frame's is 7 px or more clear of moving."""
    s = 1 << shift
    sc = _one_bin_scene(f"build_boxes@{shift}", _spread_bits(3000), shift, f"boxes clipped to a bin of {s} x {s} tiles", {})
    w = sc.width
    first = sc.expect["n"] - 3000
    big = 8.0 * s - 8.0
    at = dict(whole_bin=(24.0 * s, 24.0 * s, big), tile_row=(24.0 * s, 32.0 * s + big - 8.0, big),
              tile_column=(32.0 * s + big - 8.0, 24.0 * s, big), four_bins=(16.0 * s, 16.0 * s, 40.0),
              frame_edge=(32.0 * s - 16.0, 16.0 * (s + 4), 40.0))
    boxes = dict(whole_bin=(s, s, 2 * s, 2 * s), tile_row=(s, 2 * s - 1, 2 * s, 2 * s), tile_column=(2 * s - 1, s, 2 * s, 2 * s),
                 four_bins=(s - 3, s - 3, s + 3, s + 3), frame_edge=(2 * s - 4, s + 1, 2 * s, s + 7))
    pinned = {}
    for j, (name, lane) in enumerate(zip(BOX_PROBES, _BOX_PROBE_LANES)):
        ux, uy, radius = at[name]
        _probe(sc.records[first + lane:first + lane + 1], ux, uy, 2.5 + 0.25 * j, radius, w, w)
        pinned[first + lane] = boxes[name]
    sc.expect["probe_tiles"] = pinned
    sc.expect["bin_entries"][shift] += 3                          # four_bins lies in all four
    sc.expect["instances"] = sc.expect["n"] - 5 + sum((c - a) * (d - b) for a, b, c, d in boxes.values())
    return sc


# ------------------------------------------------------------------------------------------------ crowded bucket
def crowded_bucket(k):
    """Clusters of k consecutive binary32 patterns in a bin whose depth span two sentinels fix at 2^24 patterns (2.0 and 8.0):
    the bin's 4096 depth buckets are 8192 patterns wide (25 significant bits, shift 13).  Four clusters lie inside one bucket
    each -- at its start, its end, and twice mid-bucket -- and one is cut in half by a bucket border; 1500 single candidates in
    buckets of their own.  The fullest bucket holds exactly k."""
    width = 8192
    clusters = [(300, 0), (700, 100), (1100, 4000), (1500, width - k), (1800, width - k // 2)]
    bits = [DEPTH_2, DEPTH_2 + (1 << 24)]
    for bucket, off in clusters:
        bits += [DEPTH_2 + bucket * width + off + j for j in range(k)]
    bits += [DEPTH_2 + (2 + b) * width + 4321 for b in range(1500) if all(abs(2 + b - c) > 1 for c, _ in clusters)]
    bits = np.asarray(bits, np.int64)
    bits = bits[(np.arange(len(bits), dtype=np.int64) * PRIME) % len(bits)].astype(np.uint32)
    return _one_bin_scene(f"crowded_bucket/{k}", bits, 2, f"{k} keys in one depth bucket",
                          dict(fullest_bucket=k, bucket_shift=13, longest_run=1))


# ------------------------------------------------------------------------------------------------ slab planning
def _bucket_fill(counts, bucket_width):
    """Depth patterns: counts[b] distinct ones in bucket b (from its first pattern on); the first and the last pattern of the
    whole range are among them (they fix the bin's depth span: counts[0] and counts[-1] must not be 0)."""
    assert counts[0] > 0 and counts[-1] > 0 and max(counts) <= bucket_width
    bits = [DEPTH_2 + b * bucket_width + np.arange(c, dtype=np.int64) for b, c in enumerate(counts)]
    bits = np.concatenate(bits)
    bits[-1] = DEPTH_2 + len(counts) * bucket_width - 1
    return bits[(np.arange(len(bits), dtype=np.int64) * PRIME) % len(bits)].astype(np.uint32)


def slab_plan(kind):
    """A level-4 bin whose bucket counts decide the slab cut.  The planner (k_bin_slabs) cuts the bin's depth span into 4096
    buckets and closes a slab in front of the first bucket that would take it beyond 12288.
      exact:  buckets of 6; the first 2048 hold 12288 -- the first slab is full to the last place;
      over:   the same, but bucket 2047 holds 5 and bucket 2048 holds 2: with it the slab would hold 12289, so it closes at 12287;
      most:   buckets of 1 and of 12288 in turn, and a last one of 1: every slab holds one bucket.  The planner cuts only where a slab
              and the first bucket behind it hold more than 12288 between them, so slabs 1+2, 3+4, ... each hold more than 12288
              and n slabs need more than floor(n / 2) x 12288 candidates: 11 fit below 65535 (5 x 12288 + 6), 12 would need more
              than 73728.  kMaxSlabs = 16 can therefore not be reached through a frame, and neither can the planner's
              `remaining > MAXC` exit behind the sixteenth slab.  This is the nearest reachable case: 11 slabs, five of them full."""
    if kind in ("exact", "over"):
        counts = [6] * 3334                       # 24-bit span: 4096 buckets of 4096 patterns (the last 762 stay empty ...
        counts += [0] * (4096 - len(counts) - 1) + [1]   # ... but for the sentinel that fixes the span)
        if kind == "over":
            counts[2047], counts[2048] = 5, 2
        width = 4096
        first = 12288 if kind == "exact" else 12287
        sizes = [first, sum(counts) - first]
    else:
        counts = [1, 12288] * 5
        counts += [0] * (4096 - len(counts) - 1) + [1]
        width = 16384                             # 26-bit span: depths 2.0 .. 512.0
        sizes = [1, 12288] * 5 + [1]
    bits = _bucket_fill(counts, width)
    return _one_bin_scene(f"slab_plan/{kind}", bits, 2, f"slabs of {sizes[:3]} ... ({len(sizes)} in all)",
                          dict(slab_sizes=sizes, bucket_shift=12 if width == 4096 else 14, longest_run=1))


# ------------------------------------------------------------------------------------------------ level 1
def level1_count(n, culled=0, w=256, h=256):
    """n visible Gaussians (n = the items of the global path's level 1, and of the planes' when nothing is culled), with `culled`
    more behind the camera, dealt between them in id order; dealt round robin over every tile of the frame."""
    tx, ty = w // 16, h // 16
    i = np.arange(n, dtype=np.int64)
    t = (i * 37) % (tx * ty)
    rec = _splats(_spread_bits(n), t % tx, t // tx, w, h)
    fullest = int(np.bincount(((t // tx) >> 3) * 64 + ((t % tx) >> 3)).max())
    if culled:
        total = n + culled
        out = np.zeros((total, RECORD_FLOATS), np.float32)
        behind = np.zeros(total, bool)
        behind[(np.arange(culled, dtype=np.int64) * total) // culled] = True
        out[~behind] = rec
        dead = _splats(_spread_bits(culled), np.zeros(culled), np.zeros(culled), w, h)
        dead[:, 2] = -dead[:, 2]                  # behind the camera
        out[behind] = dead
        rec = out
    blocks = (len(rec) + L1_ITEMS - 1) // L1_ITEMS
    return LimitScene(f"level1_count/{n}+{culled}", rec, w, h, {}, f"N = {len(rec)}, V = {n}",
                      dict(n=len(rec), visible=n, l1_blocks=blocks, bin_entries={3: n}, fullest_bin={3: fullest}))


def level1_blocks(blocks):
    """N = 1024 x blocks - 1 Gaussians, all visible: exactly `blocks` level-1 blocks over the planes, the last one item short.
    A frame of 9 x 8 bins, so that 257 blocks' worth still leaves every bin below 4096 candidates (level 0, no re-run)."""
    sc = level1_count(L1_ITEMS * blocks - 1, w=1152, h=1024)
    assert sc.expect["fullest_bin"][3] <= LEVEL_LIMITS[0]
    sc.name = f"level1_blocks/{blocks}"
    sc.pins = f"{blocks} level-1 blocks"
    return sc


BIG_BOXES = ((1, 12), (2, 6), (3, 4), (1, 13), (2, 7))


def big_box(rows, cols):
    """Probe Gaussians whose bin box is exactly rows x cols bins (bins of 4 x 4 tiles), among small ones in the same wave.
    A tile box is a square around the centre, so the frame is `rows` bins high and clips it: centre in the middle of the frame's
    height, radius 8 (b - a) - 8 around the middle of tile columns [a, b), which is 7 px clear of changing either end."""
    shift, s = 2, 4
    w, h = 16 * s * 16, 16 * s * rows
    n = 640
    i = np.arange(n, dtype=np.int64)
    t = (i * 29) % (64 * 4 * rows)
    rec = _splats(_spread_bits(n), t % 64, t // 64, w, h)
    probes = [5, 64 + 63, 200, 201, 3 * 64]       # lanes 5 and 63 of two waves, two neighbours, lane 0
    a, b = s * 1, s * (1 + cols)
    radius = 8.0 * (b - a) - 8.0
    focal = w / (2.0 * np.tan(np.radians(FOV) / 2.0))
    for j, p in enumerate(probes):
        tz = 2.5 + 0.25 * j
        one = rec[p:p + 1]
        _place(one, _ndc(np.array([8.0 * (a + b)]), w), _ndc(np.array([h / 2.0 - 0.5]), h), np.array([tz]), FOV, w, h)
        one[:, 2] = -np.float32(tz)
        lam = (radius - 0.5) ** 2 / 9.0           # radius = ceil(3 sqrt(lambda)), lambda = sigma^2 + 0.3 + sqrt(0.1)
        sigma = np.sqrt(lam - 0.3 - np.sqrt(0.1))
        one[:, 55:58] = np.log(sigma * tz / focal)
        one[:, 54] = -4.0                         # faint: they cover the whole frame
    entries = n + len(probes) * (rows * cols - 1)
    per_bin = np.bincount(np.delete(((t // 64) >> 2) * 16 + ((t % 64) >> 2), probes), minlength=16 * rows).reshape(rows, 16)
    per_bin[:, 1:1 + cols] += len(probes)
    fullest = int(per_bin.max())
    return LimitScene(f"big_box/{rows}x{cols}", rec, w, h, {"GS_BIN_SHIFT": "2"}, f"bin box of {rows} x {cols} bins",
                      dict(n=n, visible=n, probes={p: (cols, rows) for p in probes}, bin_entries={shift: entries},
                           fullest_bin={shift: fullest}))


# ------------------------------------------------------------------------------------------------ blend chunks
BLEND_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193)


def blend_chunk(k):
    """Tile (2, 1) of a 96 x 64 frame holds exactly k entries and its right neighbour the next length of BLEND_LENGTHS; every
    other tile is empty.  Opacity 0.02: alpha passes the 1/255 cut at a splat's centre and 193 of them leave T = 0.02, so no
    pixel stops early and every entry of the list is walked."""
    w, h = 96, 64
    other = BLEND_LENGTHS[(BLEND_LENGTHS.index(k) + 1) % len(BLEND_LENGTHS)]
    n = k + other
    ids = (np.arange(n, dtype=np.int64) * 13) % n                 # the two tiles' ids interleave
    in_other = ids >= k
    rec = _splats(_spread_bits(n), np.where(in_other, 3, 2), np.ones(n), w, h, logit=np.log(0.02 / 0.98))
    return LimitScene(f"blend_chunk/{k}", rec, w, h, {}, f"a tile list of {k} entries",
                      dict(n=n, visible=n, tile_lists={(2, 1): k, (3, 1): other}, instances=n))


# ------------------------------------------------------------------------------------------------ guard triggers
GUARD_LIST, GUARD_RESOLVES, GUARD_PAIRS = 384, 8, 4096      # gs_blend.hip: kGuardList, kGuardMaxResolves, kGuardMaxPairs
GUARD_FRAME = 48                                            # 3 x 3 tiles; everything happens in tile (1, 1), pixels 24 .. 31 of it
GUARD_QUADRANT = (slice(24, 32), slice(24, 32))             # rows, columns of the image
_LOGIT_LO, _LOGIT_HI = np.float32(0.125), np.float32(6.0)   # final-layer logits that surely do not / surely do break


def _stacks(sites, layers, final_bits):
    """`layers` splats on the centre of each site's pixel (power = 0 there: alpha is the opacity), the sites' layers taking turns
    in depth; ids run against the depth order.  Layers 0 .. layers - 2 are weak -- together they leave T = 5e-4 -- and carry no
    red; the last layer of a site is red and has the logit whose binary32 pattern is final_bits[site].  Sites are two pixels apart:
    at that distance a 0.3 px^2 footprint stays below alpha 1/255 whatever its opacity, so a site's pixel sees its own stack only."""
    n_sites = len(sites)
    n = n_sites * layers
    e = n - 1 - np.arange(n, dtype=np.int64)                  # depth rank of id i
    layer, site = e // n_sites, e % n_sites
    px = np.asarray([p[0] for p in sites], np.float64)[site]
    py = np.asarray([p[1] for p in sites], np.float64)[site]
    rec = _splats((DEPTH_2 + e * 1000).astype(np.uint32), None, None, GUARD_FRAME, GUARD_FRAME, pixel=(px, py))
    weak = 1.0 - (5e-4) ** (1.0 / (layers - 1))
    last = layer == layers - 1
    rec[:, 54] = np.log(weak / (1.0 - weak))
    rec[last, 54] = np.asarray(final_bits, np.uint32).view(np.float32)[site[last]]
    rec[:, 6] = np.where(last, 3.0, -2.0)
    return rec, np.nonzero(last)[0][np.argsort(site[last])]     # (records, id of each site's last layer)


def breaks_at(oracle_image, sites):
    """Per site: did render.comp:83 take the break at the last layer (its red never reached the pixel)?"""
    return np.asarray([oracle_image[y, x, 0] == 0.0 for x, y in sites])


def _tuned_stacks(sites, layers, image_of):
    """Bisect every site's last logit over the binary32 patterns, against the oracle's own frame: the result is the SMALLEST
    opacity with which the reference breaks there, so its T (1 - alpha) lies within one rounding step below 1e-4."""
    lo = np.full(len(sites), _LOGIT_LO.view(np.uint32), np.int64)
    hi = np.full(len(sites), _LOGIT_HI.view(np.uint32), np.int64)
    assert not breaks_at(image_of(_stacks(sites, layers, lo)[0]), sites).any()
    assert breaks_at(image_of(_stacks(sites, layers, hi)[0]), sites).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        b = breaks_at(image_of(_stacks(sites, layers, mid)[0]), sites)
        hi, lo = np.where(b, mid, hi), np.where(b, lo, mid)
    return hi


def _guard_scene(name, pins, sites, layers, image_of, want):
    bits = _tuned_stacks(sites, layers, image_of)
    rec, last_ids = _stacks(sites, layers, bits)
    n = len(rec)
    return LimitScene(name, rec, GUARD_FRAME, GUARD_FRAME, {}, pins,
                      dict(n=n, visible=n, instances=n, tile_lists={(1, 1): n}),
                      guard=dict(sites=sites, layers=layers, final_bits=bits, last_ids=last_ids, want=want))


def guard_list(kept, image_of):
    """One pixel, `kept` layers: the break decision falls on the quadrant's kept entry number `kept` (position kept - 1 of the
    wave's list, which holds 384).  image_of(records) -> the oracle's frame at GUARD_FRAME x GUARD_FRAME."""
    return _guard_scene(f"guard_list/{kept}", f"a break decision at kept entry {kept}", [(27, 27)], kept, image_of,
                        "resolved" if kept <= GUARD_LIST else "redo")


def guard_resolves(count, image_of):
    """`count` pixels of one quadrant (of the nine at 25 / 27 / 29 in x and y), 40 layers each, every one of them with its break
    decision inside the window at its last layer: `count` replays in one quadrant, all within the first 384 kept entries."""
    sites = [(25 + 2 * (k % 3), 25 + 2 * (k // 3)) for k in range(count)]
    assert count * 40 <= GUARD_LIST
    return _guard_scene(f"guard_resolves/{count}", f"{count} replays in one quadrant", sites, 40, image_of,
                        "resolved" if count <= GUARD_RESOLVES else "redo")


def guard_pairs(kept):
    """`kept` splats on one pixel, opacity 0.8: that pixel stops at the sixth entry and its eight neighbours within 320, but the
    rest of the quadrant never blends anything and walks on, so the quadrant evaluates exactly `kept` kept entries.  No break
    decision is tuned here: beyond 4096 the quadrant is given up whatever its pixels do."""
    rec = _splats(_spread_bits(kept), None, None, GUARD_FRAME, GUARD_FRAME, logit=np.log(0.8 / 0.2),
                  pixel=(np.full(kept, 27.0), np.full(kept, 27.0)))
    return LimitScene(f"guard_pairs/{kept}", rec, GUARD_FRAME, GUARD_FRAME, {}, f"{kept} kept entries in one quadrant",
                      dict(n=kept, visible=kept, instances=kept, tile_lists={(1, 1): kept}),
                      guard=dict(sites=[(27, 27)], want="clean" if kept <= GUARD_PAIRS else "redo"))


# ------------------------------------------------------------------------------------------------ the spatial read order
def morton_order(pos):
    """gs_host_math.h's spatial_order restated: the scene ids in the order the per-frame kernels read a scene of >= GS_SPATIAL_MIN Gaussians.
    Per axis 2^21 cells over the finite coordinates' bounding box (hi = lo + 1 in binary32 on a degenerate axis), a non-finite
    coordinate in cell 0, the three cells interleaved bit by bit with x lowest, ties by id.  The cell is computed with the
    header's own binary64 operations on the binary32 values -- one subtraction each, one division, a product by 2^21 -- so it
    is the same number, not an approximation of it."""
    pos = np.asarray(pos, np.float32)
    n = len(pos)
    code = np.zeros(n, np.uint64)
    for k in range(3):
        v = pos[:, k]
        fin = np.isfinite(v)
        lo, hi = (v[fin].min(), v[fin].max()) if fin.any() else (np.float32(np.inf), np.float32(-np.inf))
        if not hi > lo:
            with np.errstate(invalid="ignore"):
                hi = np.float32(lo + np.float32(1.0))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            c = (v.astype(np.float64) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * 2097152.0
        c = np.where(fin & ~np.isnan(c), c, 0.0)              # (std::max(0.0, NaN) is 0.0)
        cell = np.minimum(2097151.0, np.maximum(0.0, c)).astype(np.uint64)
        for b in range(21):
            code |= ((cell >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + k)
    return np.lexsort((np.arange(n), code)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ preprocess, wave by wave
WAVE_COUNTS = (0, 1, 4, 5, 6, 9, 10, 11, 20, 21, 31, 32, 33, 37, 42, 43, 59, 60, 61, 63, 64)
WAVE_PLACEMENTS = ("lowest", "highest", "spread")
WAVE_TAILS = ("ends_group", "mid_group")
WAVE_RAGGED = 37                                    # valid lanes of the ragged last wave
CULL_KINDS = ("behind", "near", "off_grid")
_WAVE_FRAME = (1152, 128)
_ANCHOR = 1e7


def placement_mask(count, placement):
    """The visible lanes of a wave, as a 64-bit mask (bit l = lane l)."""
    if placement == "lowest":
        lanes = range(count)
    elif placement == "highest":
        lanes = range(WAVE - count, WAVE)
    else:
        lanes = [(k * WAVE + WAVE // 2) // count for k in range(count)]   # count 1: lane 32
    return sum(1 << l for l in lanes)


def _wave_design(order, tail):
    """Per wave, in read order: (valid lanes, mask of visible lanes).  63 waves of (placement, count), then with tail
    "mid_group" one wave of every other lane, then the ragged wave: lane 0, every third lane and its last lane -- but in
    spatial order the first and the last read slot hold the anchors, which are culled."""
    waves = [(WAVE, placement_mask(c, p)) for p in WAVE_PLACEMENTS for c in WAVE_COUNTS]
    if tail == "mid_group":
        waves.append((WAVE, sum(1 << l for l in range(1, WAVE, 2))))
    ragged = sum(1 << l for l in range(0, WAVE_RAGGED, 3)) | 1 << (WAVE_RAGGED - 1)
    if order == "spatial":
        ragged &= ~(1 << (WAVE_RAGGED - 1))
    waves.append((WAVE_RAGGED, ragged))
    assert waves[0][1] & 1 == 0                     # read slot 0 is culled in either order
    return waves


def wave_patterns(order, tail="ends_group"):
    """k_preprocess at every count of visible lanes.  One wave per (count, placement), counts WAVE_COUNTS -- the steps of the
    LDS-DMA fetch of the SH blocks (5 | 6 and 10 | 11 Gaussians per instruction, 32 | 33 per round, 60 lanes that fetch) and of
    the record store -- placed in the lowest lanes, the highest lanes, or spread over the wave; then a ragged wave of 37 lanes,
    which ends the last workgroup (tail "ends_group": 64 waves) or is followed by three waves without any Gaussian ("mid_group":
    one more wave first, so that the ragged one is the first of its workgroup).  The culled lanes of a wave take the kernel's
    exits in turn: behind the camera, inside the near cut (z = -0.19), a tile box that is empty (centred three frame heights off
    the grid).

    The visible ones are _splats with a 0.5 px footprint (radius 3 still, one tile each; the antialiased mode's factor is then
    0.45 instead of 3e-4, so its frames are not black) and 45 SH rest coefficients ~ N(0, 0.6) from a fixed seed: a swapped
    block or 16-byte chunk changes the colour.

    order "spatial" (GS_SPATIAL_MIN=0): the Gaussian in read slot j has scene id sigma(j) = (PRIME j + 12345) mod N, and the
    positions are such that the order of gs_host_math.h's spatial_order IS sigma.  World x strictly increases with the read slot (the splat's
    pixel is then computed from it and its own depth: depths span 4096 binary32 patterns, which moves a pixel by < 0.3 px);
    two culled anchors at y = z = -9999995 and +10000005 (read slots 0 and N - 1) make the y and z cells 9.5 units wide with
    0 near the middle of one, so the whole cluster shares its y and its z cell and the code orders by x alone."""
    w, h = _WAVE_FRAME
    waves = _wave_design(order, tail)
    n = sum(v for v, _ in waves)
    valid_before = np.cumsum([0] + [v for v, _ in waves])
    vis = np.zeros(n, bool)
    kind = np.full(n, -1)
    for wv, (valid, mask) in enumerate(waves):
        lanes = np.arange(valid)
        on = np.array([(mask >> l) & 1 for l in range(valid)], bool)
        vis[valid_before[wv] + lanes] = on
        off = lanes[~on]
        kind[valid_before[wv] + off] = np.arange(len(off)) % 3
    j = np.arange(n, dtype=np.int64)
    nvis = int(vis.sum())
    bits = np.full(n, DEPTH_2, np.uint32)
    bits[vis] = _spread_bits(nvis, span=4096)
    tz = bits.view(np.float32).astype(np.float64)
    tan_x = np.tan(np.radians(float(np.float32(FOV))) / 2.0)
    cols = w // 16
    u = j * cols / n                                             # strictly increasing: the column and the place inside it
    nominal = 16.0 * np.floor(u) + 5.5 + 4.0 * (u - np.floor(u))
    x_world = _ndc(nominal, w) * 2.0 * tan_x
    px = ((x_world / (tz * tan_x) + 1.0) * w - 1.0) / 2.0
    assert (np.abs(px - nominal) < 0.3).all()
    py = 16.0 * ((j * 5) % (h // 16)) + 7.5 + ((j * 3) % 5 - 2)
    rec = _splats(bits, None, None, w, h, pixel=(px, py))
    focal = w / (2.0 * tan_x)
    rec[:, 55:58] = np.log(0.5 * tz / focal)[:, None]            # 0.5 px: lambda = 0.25 + 0.3 + sqrt(0.1), radius ceil(2.79)
    rec[:, 9:54] = (0.6 * np.random.default_rng(20240607).normal(size=(n, 45))).astype(np.float32)
    rec[kind == 0, 2] = np.float32(2.0)
    rec[kind == 1, 2] = np.float32(-0.19)
    rec[kind == 2, 1] = np.float32(6.0 * tan_x * h / w)          # NDC y = -3 at depth 2
    env = {"GS_SPATIAL_MIN": "1000000000"}
    sigma = j
    if order == "spatial":
        env = {"GS_SPATIAL_MIN": "0"}
        for slot, a in ((0, np.float32(-_ANCHOR + 5.0)), (n - 1, np.float32(_ANCHOR + 5.0))):
            assert not vis[slot]
            rec[slot, 1:3] = (a, a)                               # (x stays: the least and the greatest of the scene)
        sigma = (j * PRIME + 12345) % n
        out = np.empty_like(rec)
        out[sigma] = rec
        rec = out
        assert np.array_equal(morton_order(rec[:, :3]), sigma)
    masks = [m for _, m in waves]
    e = dict(n=n, visible=nvis, wave_masks=masks, ragged_lanes=WAVE_RAGGED,
             placements={p: list(WAVE_COUNTS) for p in WAVE_PLACEMENTS}, cull_kinds_in_every_wave=True, tiles_per_visible=1,
             waves_after_the_ragged_one=(-len(waves)) % (PRE_BLOCK // WAVE))
    return LimitScene(f"wave_patterns/{order}/{tail}", rec, w, h, env, f"{len(waves)} waves of k_preprocess, {nvis} of {n} visible", e)


def read_order(scene):
    """The scene ids in the order k_preprocess reads them."""
    if scene.env.get("GS_SPATIAL_MIN") == "0":
        return morton_order(scene.records[:, :3])
    return np.arange(len(scene.records), dtype=np.uint32)


def _measure_waves(scene, ref, m):
    order = read_order(scene)
    n = len(order)
    tiles = ref["tiles"][order]
    lanes = np.zeros(-(-n // WAVE) * WAVE, bool)
    lanes[:n] = tiles != 0
    m["wave_masks"] = [sum(1 << l for l in np.nonzero(row)[0].tolist()) for row in lanes.reshape(-1, WAVE)]
    m["ragged_lanes"] = n % WAVE
    m["waves_after_the_ragged_one"] = (-len(m["wave_masks"])) % (PRE_BLOCK // WAVE)
    m["placements"] = {p: [c for c in WAVE_COUNTS if placement_mask(c, p) in m["wave_masks"][:-1]] for p in WAVE_PLACEMENTS}
    m["tiles_per_visible"] = int(tiles.max())
    # the exit a culled Gaussian takes, from its record: behind (z > 0), the near cut (0 > z >= -0.2), else its box
    z = scene.records[order, 2]
    kind = np.where(z > 0, 0, np.where(z >= -0.2, 1, 2))
    ok = True
    for wv in range(len(m["wave_masks"])):
        k = kind[wv * WAVE:(wv + 1) * WAVE][tiles[wv * WAVE:(wv + 1) * WAVE] == 0]
        ok &= len(k) < 3 or set(k.tolist()) == {0, 1, 2}
    m["cull_kinds_in_every_wave"] = bool(ok)


def dense_lists_full():
    """262144 Gaussians, all visible, with the dense lists on: the smallest scene in which every one of the 256 lists is full to
    its last slot -- vis_region_slots = 1024 = the four workgroups of 256 that append to a list (region = (i / 256) % 256)."""
    sc = level1_count(VIS_REGIONS * L1_ITEMS, w=1152, h=1024)
    assert sc.expect["fullest_bin"][3] <= LEVEL_LIMITS[0]
    sc.name = "dense_lists_full"
    sc.env = {"GS_L1_DENSE_MIN": "0"}
    sc.pins = "256 dense lists of 1024 entries in 1024 slots"
    sc.expect["list_fill"] = dict(lists=VIS_REGIONS, slots=L1_ITEMS, fewest=L1_ITEMS, most=L1_ITEMS)
    return sc


def vis_region_slots(n):
    """gs_bin_l1.hip: vis_region_slots."""
    groups = (n + PRE_BLOCK - 1) // PRE_BLOCK
    slots = (groups + VIS_REGIONS - 1) // VIS_REGIONS * PRE_BLOCK
    return L1_ITEMS if slots == 0 else (slots + L1_ITEMS - 1) // L1_ITEMS * L1_ITEMS


# ------------------------------------------------------------------------------------------------ the global path's grid
RADIX_SIZES = (524288, 524289, 1048577, 1572865, 2097152, 2097153)
RADIX_SMALL_V = (2047, 2048, 2049, 4097)
_RADIX_FRAME = (1152, 1024)


def radix_grid(n):
    """(blocks, entries per thread of k_radix_scan) of a scene of n Gaussians: gs_renderer.cpp, gs_radix.hip."""
    blocks = max(1, min(SORT_MAX_BLOCKS, (n + SORT_TILE - 1) // SORT_TILE))
    return blocks, (blocks + SCAN_THREADS - 1) // SCAN_THREADS


def radix_tiles_of_block(count, blocks):
    """[t0, t1) per block over `count` keys: t0 = b ntiles / blocks (k_radix_hist, k_radix_scatter)."""
    ntiles = (count + SORT_TILE - 1) // SORT_TILE
    b = np.arange(blocks + 1, dtype=np.int64)
    t = b * ntiles // blocks
    return t[:-1], t[1:]


def _radix_whole_tiles(n):
    """The tiles of the first pass (2048 ids each) that are visible as a whole.  With one tile per block EVERY tile border is a
    change of the owning block, and whole tiles on both sides of each of them would be the whole scene: taken are the first two
    tiles, the last two (the last one ragged), both sides of the block numbers 256, 512 and 768 -- where k_radix_scan's threads
    take one more entry each -- and the tiles of a block that owns two, with the block before it."""
    blocks, _ = radix_grid(n)
    ntiles = (n + SORT_TILE - 1) // SORT_TILE
    t0, t1 = radix_tiles_of_block(n, blocks)
    tiles = {0, 1, ntiles - 2, ntiles - 1}
    for b in (256, 512, 768):
        if b < blocks:
            tiles |= {int(t1[b - 1]) - 1, int(t0[b])}
    for b in np.nonzero(t1 - t0 > 1)[0].tolist():
        tiles |= set(range(int(t0[b]) - 1, int(t1[b])))
    return sorted(tiles)


def radix_blocks(n, v=None):
    """n Gaussians behind the camera but for the visible ones, on the global path: the radix passes' grid is sized by n (blocks =
    min(1024, ceil(n / 2048)): RADIX_SIZES give 256, 257, 513, 769, 1024 and 1024 blocks over 1025 tiles) while the passes after the
    first run over the V visible keys only, so that most blocks own no tile.
    v None: visible are every 97th id and the whole tiles of _radix_whole_tiles (tens of thousands).  v given: exactly v ids spread
    evenly from the first id to the last (RADIX_SMALL_V: the later passes' single tile one key short, full, and one and two tiles
    with one key more).
    Depths: distinct patterns scrambled against the ids; the eight patterns whose three low bytes are each 0x00 or 0xFF, each in
    three tiles (so equal depths in different tiles and blocks); five more groups of five equal depths, each group's ids a fifth
    of the scene apart; and, where a block owns two tiles, the last id (alone in the block's second tile) at the depth of an id of
    the block's first tile, so that the carry between a block's tiles moves a cursor that is then used, in every pass."""
    w, h = _RADIX_FRAME
    blocks, per = radix_grid(n)
    ntiles = (n + SORT_TILE - 1) // SORT_TILE
    if v is None:
        mask = np.zeros(n, bool)
        mask[::97] = True
        for t in _radix_whole_tiles(n):
            mask[t * SORT_TILE:(t + 1) * SORT_TILE] = True
        ids = np.nonzero(mask)[0]
    else:
        ids = (np.arange(v, dtype=np.int64) * (n - 1)) // (v - 1)
    nv = len(ids)
    bits = _spread_bits(nv).astype(np.int64)
    third = nv // 3
    for c in range(8):                                           # 0x40 bb bb bb: depths 2.0 .. 2.99
        pattern = DEPTH_2 | (0xFF0000 if c & 4 else 0) | (0xFF00 if c & 2 else 0) | (0xFF if c & 1 else 0)
        for k in range(3):
            bits[k * third + 100 + 37 * c] = pattern
    for g in range(5):
        bits[(g * 7 + 3 + np.arange(5) * (nv // 5)) % nv] = DEPTH_2 + 7777 * (g + 1) + 1
    t0, t1 = radix_tiles_of_block(n, blocks)
    two = np.nonzero(t1 - t0 > 1)[0]
    if len(two) and v is None:
        first_tile = int(t0[two[0]])
        bits[-1] = bits[np.searchsorted(ids, first_tile * SORT_TILE + 5)]   # (the whole tile is visible: that id is)
    i = np.arange(nv, dtype=np.int64)
    t = (i * 37) % ((w // 16) * (h // 16))
    rec = np.zeros((n, RECORD_FLOATS), np.float32)
    rec[:, 2] = 3.0                                              # behind the camera
    rec[:, 55:58] = np.float32(np.log(3e-5))
    rec[:, 58] = 1.0
    rec[ids] = _splats(bits.astype(np.uint32), t % (w // 16), t // (w // 16), w, h)
    e = dict(n=n, visible=nv, radix=dict(blocks=blocks, per=per, blocks_owning_two_tiles=int(len(two)),
                                         tiles_of_the_later_passes=(nv + SORT_TILE - 1) // SORT_TILE),
             low_byte_patterns_in_several_tiles=8, equal_depths_across_blocks=True)
    if len(two) and v is None:
        e["radix"]["carry_shares_a_digit"] = [True] * 4
    return LimitScene(f"radix_blocks/{n}/{'grid' if v is None else v}", rec, w, h, {}, f"N = {n}: {blocks} blocks, V = {nv}", e)


def _measure_radix(scene, ref, m):
    n = len(ref["tiles"])
    blocks, per = radix_grid(n)
    t0, t1 = radix_tiles_of_block(n, blocks)
    two = np.nonzero(t1 - t0 > 1)[0]
    ids = np.nonzero(ref["tiles"])[0]
    bits = ref["attr"]["depth"][ids].view(np.uint32).astype(np.int64)
    m["radix"] = dict(blocks=blocks, per=per, blocks_owning_two_tiles=int(len(two)),
                      tiles_of_the_later_passes=(len(ids) + SORT_TILE - 1) // SORT_TILE)
    if "carry_shares_a_digit" in scene.expect["radix"]:
        tile = ids // SORT_TILE
        first = t0[two[0]] if len(two) else -2                   # (no such block: nothing shares anything)
        a, b = bits[tile == first], bits[tile == first + 1]
        m["radix"]["carry_shares_a_digit"] = [bool(set(((a >> s) & 255).tolist()) & set(((b >> s) & 255).tolist())) for s in (0, 8, 16, 24)]
    tile = ids // SORT_TILE
    low = bits & 0xFFFFFF
    combos = [(0xFF0000 if c & 4 else 0) | (0xFF00 if c & 2 else 0) | (0xFF if c & 1 else 0) for c in range(8)]
    m["low_byte_patterns_in_several_tiles"] = sum(len(set(tile[low == p].tolist())) > 1 for p in combos)
    order = np.lexsort((ids, bits))
    sb, st = bits[order], tile[order]
    block_of_tile = np.searchsorted(t1, np.arange(int(t1[-1])), side="right")
    same = sb[1:] == sb[:-1]
    m["equal_depths_across_blocks"] = bool((same & (st[1:] != st[:-1]) & (block_of_tile[st[1:]] != block_of_tile[st[:-1]])).any())


# ================================================================================================ measuring
def tiles_across(pixels):
    return (pixels + 15) // 16


def grid_fits(tx, ty, s):
    return ((tx - 1) >> s) + 1 <= 32 and ((ty - 1) >> s) + 1 <= 32


def base_shift(tx, ty, min_shift):
    s = max(2, min_shift)
    while not grid_fits(tx, ty, s):
        s += 1
    return s


def can_refine(w, h, min_shift):
    tx, ty = tiles_across(w), tiles_across(h)
    s = base_shift(tx, ty, min_shift)
    return 2 < s <= 5 and grid_fits(tx, ty, s - 1)


def bin_boxes(ref, shift):
    """Per visible Gaussian: (ids, x0, y0, x1, y1) of its box in bins, upper bounds exclusive (gs_bin.h: l1_item)."""
    ids = np.nonzero(ref["tiles"])[0]
    box = ref["attr"]["aabb"][ids].astype(np.int64)
    return ids, box[:, 0] >> shift, box[:, 1] >> shift, ((box[:, 2] - 1) >> shift) + 1, ((box[:, 3] - 1) >> shift) + 1


def bin_members(ref, shift):
    """{(bx, by): ids of the bin's candidates, ascending}."""
    ids, x0, y0, x1, y1 = bin_boxes(ref, shift)
    out = {}
    for g, a, b, c, d in zip(ids.tolist(), x0.tolist(), y0.tolist(), x1.tolist(), y1.tolist()):
        for y in range(b, d):
            for x in range(a, c):
                out.setdefault((x, y), []).append(g)
    return {k: np.asarray(v, np.int64) for k, v in out.items()}


def measure(scene, ref):
    """The quantities of scene.expect, recomputed from the oracle's stages alone."""
    m = {"n": len(ref["tiles"]), "visible": int((ref["tiles"] != 0).sum())}
    e = scene.expect
    if "wave_masks" in e:
        _measure_waves(scene, ref, m)
    if "radix" in e:
        _measure_radix(scene, ref, m)
    if "list_fill" in e:
        region = (np.nonzero(ref["tiles"])[0] // PRE_BLOCK) % VIS_REGIONS
        fill = np.bincount(region, minlength=VIS_REGIONS)
        m["list_fill"] = dict(lists=len(fill), slots=vis_region_slots(m["n"]), fewest=int(fill.min()), most=int(fill.max()))
    if "instances" in e:
        m["instances"] = len(ref["keys"])
    if "l1_blocks" in e:
        m["l1_blocks"] = (m["n"] + L1_ITEMS - 1) // L1_ITEMS
    if "bin_entries" in e:
        m["bin_entries"] = {}
        for s in e["bin_entries"]:
            _, x0, y0, x1, y1 = bin_boxes(ref, s)
            m["bin_entries"][s] = int(((x1 - x0) * (y1 - y0)).sum())
    if "probes" in e:
        ids, x0, y0, x1, y1 = bin_boxes(ref, scene.min_shift)
        at = {int(g): k for k, g in enumerate(ids)}
        m["probes"] = {p: (int(x1[at[p]] - x0[at[p]]), int(y1[at[p]] - y0[at[p]])) for p in e["probes"]}
        m["largest_other_box"] = int(np.delete((x1 - x0) * (y1 - y0), [at[p] for p in e["probes"]]).max())
    if "probe_tiles" in e:
        box = ref["attr"]["aabb"].astype(np.int64)
        m["probe_tiles"] = {p: tuple(int(v) for v in box[p]) for p in e["probe_tiles"]}
        area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        m["largest_other_tile_box"] = int(np.delete(area, list(e["probe_tiles"])).max())
    if "longest_tile_list" in e:
        b = ref["boundaries"].astype(np.int64)
        tx = tiles_across(scene.width)
        lens = b[1::2] - b[0::2]
        t = int(lens.argmax())
        m["longest_tile_list"] = ((t % tx, t // tx), int(lens[t]))
    if "bin_counts" in e:
        m["bin_counts"] = {}
        for s, bins in e["bin_counts"].items():
            members = bin_members(ref, s)
            m["bin_counts"][s] = {k: len(members.get(k, ())) for k in bins}
            m["tile_columns_of_the_last_bin"] = tiles_across(scene.width) - ((tiles_across(scene.width) - 1) >> s << s)
    if "tile_lists" in e:
        b = ref["boundaries"].astype(np.int64)
        tx = tiles_across(scene.width)
        lens = b[1::2] - b[0::2]
        m["tile_lists"] = {(int(t % tx), int(t // tx)): int(lens[t]) for t in np.nonzero(lens)[0]}
    if "fullest_bin" in e:
        m["fullest_bin"] = {}
        for s in e["fullest_bin"]:
            members = bin_members(ref, s)
            key = max(members, key=lambda k: len(members[k]))
            m["fullest_bin"][s] = len(members[key])
            if s != scene.min_shift:
                continue
            ids = members[key]
            bits = ref["attr"]["depth"][ids].view(np.uint32).astype(np.int64)
            order = np.lexsort((ids, bits))
            sb = bits[order]
            if "longest_run" in e:
                starts = np.nonzero(np.r_[True, sb[1:] != sb[:-1]])[0]
                lens = np.diff(np.r_[starts, len(sb)])
                m["longest_run"] = int(lens.max())
                if "run_start" in e:
                    m["run_start"] = int(starts[lens.argmax()])
            if "bucket_shift" in e:
                span = int(sb[-1] - sb[0])
                nbits = span.bit_length()
                sh = nbits - 12 if nbits > 12 else 0
                m["bucket_shift"] = sh
                bucket = (sb - sb[0]) >> sh
                counts = np.bincount(bucket, minlength=MSD_BUCKETS)
                if "fullest_bucket" in e:
                    m["fullest_bucket"] = int(counts.max())
                if "slab_sizes" in e:
                    m["slab_sizes"] = plan_slabs(counts)
    return m


def plan_slabs(counts):
    """The slab cut of k_bin_slabs over a bin's bucket histogram: a slab takes buckets while it stays <= 12288.  Returns the
    slabs' sizes, or None where the planner gives up (a bucket beyond a slab, more than 16 slabs)."""
    if counts.max() > SLAB_MAX:
        return None
    sizes, cur = [], 0
    for c in counts.tolist():
        if cur + c > SLAB_MAX:
            sizes.append(cur)
            cur = 0
        cur += c
    sizes.append(cur)
    return sizes if len(sizes) <= MAX_SLABS else None


def predict(scene, forced=False, sort_path=0):
    """What a FRESH renderer's stats say after one frame of the scene (gs_depth_policy.h, restated): the level it ends at, the
    re-runs on the way, the bin edge, the fullest bin.  forced: gs_set_sort_path(2); "error" where that mode gives up, and
    "bin too full" where it gives up over a bin of 16 x 16 tiles or more.  sort_path 1: gs_set_sort_path(1), the global path at once.
    Bins of 16 x 16 tiles or more (shift >= 4) are ordered by k_bin_build at every bin-local level: such a bin fits a
    bin-local level if and only if it holds <= 16384, at level 0 already, and one that does not has no level 4 to go to -- it
    is refined or goes straight to the global path."""
    return _walk(scene, forced, sort_path)[0]


def attempts(scene, forced=False, sort_path=0):
    """[(bin shift, level)] of every attempt predict() passes through, the frame that finally retires (or fails) last."""
    return _walk(scene, forced, sort_path)[1]


def _walk(scene, forced, sort_path):
    tx, ty = tiles_across(scene.width), tiles_across(scene.height)
    shift = base_shift(tx, ty, scene.min_shift)
    level, retries, refined = (GLOBAL_LEVEL if sort_path == 1 else 0), 0, False
    tried = []
    while True:
        tried.append((shift, level))
        fullest = scene.expect["fullest_bin"][shift]
        one_size = shift >= ONE_SIZE_SHIFT
        if one_size:
            fits = level == GLOBAL_LEVEL or fullest <= BUILD_MAX
        else:
            fits = level == GLOBAL_LEVEL or (fullest <= LEVEL_LIMITS[level] and not (level == SLAB_LEVEL and scene.slabs_fail))
        if fits:
            return dict(sort_level=level, sort_path=1 if level == GLOBAL_LEVEL else 2, retries=retries, bin_tiles=1 << shift,
                        max_bin_entries=fullest, num_bin_entries=scene.expect["bin_entries"][shift]), tried
        wanted = level + 1
        while wanted < GLOBAL_LEVEL and fullest > LEVEL_LIMITS[wanted]:
            wanted += 1
        if one_size:
            wanted = GLOBAL_LEVEL
        if wanted >= SLAB_LEVEL and not refined and can_refine(scene.width, scene.height, scene.min_shift):
            refined, shift, level = True, shift - 1, max(level, SLAB_LEVEL - 1)
        else:
            if forced and wanted >= GLOBAL_LEVEL:
                return ("bin too full" if one_size else "error"), tried
            level = max(level, wanted)
        retries += 1


# ================================================================================================ the one-pass level 1
MAX_INSTANCES = (1 << 30) - 4096                    # gs_internal.h: kMaxInstances
ONE_PASS_MAX_SHIFT = 3                              # gs_renderer.cpp: the path needs bins of <= 8 x 8 tiles (and a bin-local level)
WIDE_RATIO = 8                                      # gs_depth_policy.h: L1FusedPolicy::kWideRatio


def candidate_capacity(n, env=None):
    """gs_renderer::init restated: the level-1 candidates the candidate buffer of a fresh renderer over a scene of n Gaussians
    holds -- min(max(2^18, 2 n), max(2^20, 8 n)), capped at the instance maximum -- under the two test knobs of `env`."""
    env = env or {}
    want = max(1 << 20, 8 * n)
    if "GS_INITIAL_CAPACITY" in env:
        want = max(256, int(env["GS_INITIAL_CAPACITY"]))
    capacity = min(want, MAX_INSTANCES)
    cand = max(1 << 18, 2 * n)
    if "GS_INITIAL_CAND_CAPACITY" in env:
        cand = max(256, int(env["GS_INITIAL_CAND_CAPACITY"]))
    elif "GS_INITIAL_CAPACITY" in env:
        cand = min(cand, want)
    return min(cand, capacity)


def screen_bins(width, height, shift):
    """The on-screen bins of a frame with bins of 2^shift tiles (gs_depth_policy.h: bin_geometry)."""
    return (((tiles_across(width) - 1) >> shift) + 1) * (((tiles_across(height) - 1) >> shift) + 1)


def region_cap(cand_capacity, bins):
    """gs_depth_policy.h: L1FusedPolicy::region_cap -- the records of the candidate buffer every on-screen bin owns."""
    return cand_capacity // bins if bins else 0


def one_pass_final(want):
    """Does the frame that finally retires take the one-pass level 1 when the switch forces it (gs_set_level1_fused(1), a scene
    below the dense-list threshold)?  `want`: predict()'s result.  Bin-local, with bins of at most 8 x 8 tiles."""
    return isinstance(want, dict) and want["sort_path"] == 2 and want["bin_tiles"] <= 1 << ONE_PASS_MAX_SHIFT


# what tests/test_gpu_limits.py runs with one_pass=True, by builder (test_limit_scenes.py checks every one of them on the CPU)
ONE_PASS_SLAB_COUNTS = (16385, 65534, 65535)
ONE_PASS_L1_COUNTS = tuple((n, culled) for n in (255, 256, 257, 1025) for culled in (0, 300))
ONE_PASS_REFUSAL = (1025, 4)                        # build_size: bins of 16 x 16 tiles -- the switch does not engage


def one_pass_scenes():
    """(scene, the fullest bin must FILL its region exactly) of every limit scene that runs on the one-pass level 1."""
    for lim in LEVEL_LIMITS[:4]:
        for d in (-1, 0, 1):
            yield level2_size(lim + d), False
    yield level2_size(16385, shift=3), False
    for c in ONE_PASS_SLAB_COUNTS:
        yield level2_size(c), False
    yield level2_size(65536), True
    for length in (64, 65, 66, 67):
        for place in RUN_PLACES:
            yield equal_run(length, place, slab=False), False
            yield equal_run(length, place, slab=True), False
    for k in (63, 64, 65, 66):
        yield crowded_bucket(k), False
    for kind in ("exact", "over", "most"):
        yield slab_plan(kind), False
    for rows, cols in BIG_BOXES:
        yield big_box(rows, cols), False
    for n, culled in ONE_PASS_L1_COUNTS:
        yield level1_count(n, culled), False
    yield build_size(*ONE_PASS_REFUSAL), False


def wide_ratio(extra):
    """The wide-splat exit of the one-pass level 1 (L1FusedPolicy: E1 > 8 V).  320 probes (big_box's technique, through _probe) on
    a frame of 8 x 8 bins of 4 x 4 tiles, each of radius 120: a tile box 16 tiles wide, which is four bins, and -- centred on the
    frame's top or bottom edge, which clips it -- 8 tiles high, which is two.  Every visible Gaussian touches exactly 2 x 4 bins:
    E1 = 8 V.  extra: the last one has radius 88 around the middle of tiles [8, 20) instead, 12 x 12 tiles or 3 x 3 bins: E1 = 8 V + 1.
    Every box edge that is not the frame's is 7 px or more clear of moving."""
    w = h = 512
    n = 320
    i = np.arange(n, dtype=np.int64)
    rec = _splats(_spread_bits(n), i % 32, i % 32, w, h)
    for j in range(n):
        a = 4 * (j % 5)                                          # tile columns [a, a + 16): bins a / 4 .. a / 4 + 3
        _probe(rec[j:j + 1], 16.0 * a + 128.0, 0.0 if (j // 5) % 2 == 0 else float(h), 2.5 + 0.005 * j, 120.0, w, h)
    if extra:
        _probe(rec[n - 1:n], 224.0, 224.0, 2.5 + 0.005 * (n - 1), 88.0, w, h)   # the middle of tiles [8, 20), both ways
    e1 = WIDE_RATIO * n + (1 if extra else 0)
    per_bin = np.zeros((8, 8), np.int64)
    boxes = {}
    for j in range(n):
        a, top = j % 5, (j // 5) % 2 == 0
        box = (a, 0 if top else 6, a + 4, 2 if top else 8)
        if extra and j == n - 1:
            box = (2, 2, 5, 5)
        boxes[j] = (box[2] - box[0], box[3] - box[1])
        per_bin[box[1]:box[3], box[0]:box[2]] += 1
    return LimitScene(f"wide_ratio/{'over' if extra else 'at'}", rec, w, h, {"GS_BIN_SHIFT": "2", "GS_SPATIAL_MIN": "0"},
                      f"E1 = 8 V{' + 1' if extra else ''}",
                      dict(n=n, visible=n, bin_entries={2: e1}, fullest_bin={2: int(per_bin.max())},
                           probes={j: boxes[j] for j in (0, 7, 158, n - 1)}))

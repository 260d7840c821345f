"""Small scenes for gs_project_backward's tests, shared by the CPU and the GPU half: records (62-float PLY rows) and a frame size.

BRANCH (64 x 48, default camera: t = (x, -y, -z)): one Gaussian per decision the definition takes from the frame --
    0, 1   t0/t2 = +-1.8 tan_fovx: 1.38 times the clamp's limit 1.3 tan_fovx, on either side; 0.7 units wide at depth 4, a footprint
           of some 40 px radius, so that the image still sees them;
    2      t0/t2 = 0.3 tan_fovx: 0.23 of the limit, well inside;
    3, 4   t1/t2 = +-1.8 tan_fovy, the same for the other axis;
    5      an SH block that drives channel 0 to 0.5 - 0.85 - |rest| < -0.2: the record holds r = 0;
    6      its twin with the DC term's sign flipped: r > 0.7;
    7      a needle along world x with two scales that activate to exactly 0 and the identity rotation: every term of cov11 and cov01
           is an exact zero in any association, so the binary64 det_raw is 0 -- comp is the constant 0 in antialiased frames."""
import numpy as np

RECORD_FLOATS = 62
BRANCH_FRAME = (64, 48)
BRANCH_BEYOND_X, BRANCH_INSIDE_X, BRANCH_BEYOND_Y, BRANCH_RED_OFF, BRANCH_RED_ON, BRANCH_NEEDLE = (0, 1), 2, (3, 4), 5, 6, 7


def branch_records():
    w, h = BRANCH_FRAME
    tan_x = np.tan(np.radians(45.0) / 2.0)
    tan_y = tan_x * h / w
    tz = 4.0
    n = 8
    rng = np.random.default_rng(77)
    rec = np.zeros((n, RECORD_FLOATS), np.float32)
    rec[:, 2] = -tz - 0.01 * np.arange(n)
    rec[:, 6:9] = 0.8 * rng.standard_normal((n, 3))
    rec[:, 9:54] = 0.05 * rng.standard_normal((n, 45))
    rec[:, 54] = rng.uniform(-1.0, 1.0, n)
    rec[:, 55:58] = np.log(0.7) + 0.2 * rng.standard_normal((n, 3))
    rec[:, 58:62] = rng.standard_normal((n, 4))
    rec[0, 0], rec[1, 0], rec[2, 0] = 1.8 * tan_x * tz, -1.8 * tan_x * tz, 0.3 * tan_x * tz
    rec[3, 1], rec[4, 1] = 1.8 * tan_y * tz, -1.8 * tan_y * tz
    for g in (2, 5, 6, 7):
        rec[g, 55:58] = np.log(0.15) + 0.2 * rng.standard_normal(3)
    rec[5, 0:2], rec[6, 0:2], rec[7, 0:2] = (-0.4, 0.3), (0.5, -0.2), (0.1, 0.1)
    rec[5, 6], rec[6, 6] = -3.0, 3.0
    rec[7, 55:58] = (np.log(0.3), -200.0, -200.0)
    rec[7, 58:62] = (1.0, 0.0, 0.0, 0.0)
    return rec


def random_gradients(n, seed=7):
    """float64 input gradients for every Gaussian, all nine record values: colour (n, 3), opacity (n,), conic (n, 3), uv (n, 2)."""
    rng = np.random.default_rng(seed)
    return dict(colour=rng.standard_normal((n, 3)), opacity=rng.standard_normal(n), conic=rng.standard_normal((n, 3)),
                uv=rng.standard_normal((n, 2)))

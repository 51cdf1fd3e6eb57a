"""TEST INFRASTRUCTURE ONLY -- the restated blur / elastic stages of the SimCLR image chain.

A NumPy restatement, from explicit inputs, of the two stage kinds avd_augment_views_x adds to the
stage-by-stage augmentation kernel (csrc/augment.hip, include/avdino.h):

* ``blur``     torchvision GaussianBlur: w[i] = exp(-0.5 (x_i / sigma)^2) normalised, the 2-D
               kernel outer(w, w), reflect padding without edge repeat, direct K x K sum;
* ``elastic``  torchvision ElasticTransform.get_params + elastic_transform (bilinear, fill 0): two
               noise fields in [-1, 1) smoothed by the same Gaussian with K_e = int(8 sigma + 1)
               taps (made odd), a bilinear zero-padded resample at
               ix = x + b_x alpha W / (2H), iy = y + b_y alpha H / (2W), times the same resample
               of an all-ones mask.

Every function takes ``dt``: float64 is the yardstick (tests/test_simclr_aug_cpu.py pins it to
torch's own pad / conv2d / grid_sample composed the way torchvision composes them); float32
evaluates the *same* restatement, in the kernel's operation order, and gives the tests their
tolerance (the float32 result's distance from the float64 one) -- and, where no transcendental is
involved (a 1-tap elastic smoothing), the kernel's exact bits.

``noise_fields`` reproduces the kernel's counter hash bit for bit:
    u = (mix64(seed ^ mix64(rec << 32 | 0x80000000 | field << 16 | pixel)) >> 40) * 2^-24,
    n = 2u - 1,   field 0 = x, 1 = y,   pixel = y * W + x.
"""
import numpy as np

from oracle import augment as OA

K_ELASTIC, K_BLUR = 9, 10
X_SIGMA, X_K, X_ALPHA, X_ESIGMA = 0, 1, 2, 3     # include/avdino.h AVD_AUG_X*


def noise_fields(seed, rid, H, W):
    """The elastic stage's two noise fields (n_x, n_y), float32 [H, W], exactly as drawn by the
    kernel for record ``rid``."""
    pix = np.arange(H * W, dtype=np.uint64)
    out = []
    with np.errstate(over="ignore"):
        for field in (0, 1):
            low = np.uint64(0x80000000) | np.uint64(field << 16) | pix
            key = (np.uint64(rid) << np.uint64(32)) | low
            r = OA._mix64(np.uint64(seed) ^ OA._mix64(key))
            u = (r >> np.uint64(40)).astype(np.float32) * np.float32(5.9604644775390625e-8)
            out.append((np.float32(2.0) * u - np.float32(1.0)).reshape(H, W))
    return out[0], out[1]


def elastic_taps(sigma):
    """int(8 sigma + 1), +1 if even, in float32 (the record holds a float32 sigma)."""
    ke = int(np.float32(8.0) * np.float32(sigma) + np.float32(1.0))
    return ke if ke & 1 else ke + 1


def gauss_taps(K, sigma, dt=np.float64):
    """Normalised 1-D Gaussian, summed in index order."""
    sigma = dt(sigma)
    x = (np.arange(K) - K // 2).astype(dt) / sigma
    e = np.exp(dt(-0.5) * (x * x)).astype(dt)
    s = dt(0)
    for v in e:
        s = s + v
    return (e / s).astype(dt)


def reflect(i, n):
    """torch's reflect padding index: -1 -> 1, n -> n - 2."""
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def blur(img, sigma, K, dt=np.float64):
    """GaussianBlur(K, sigma) of img [H, W]: direct K x K sum, taps in row-major order."""
    H, W = img.shape
    assert K % 2 == 1 and K // 2 <= min(H, W) - 1
    img = img.astype(dt)
    w = gauss_taps(K, sigma, dt)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r = K // 2
    acc = np.zeros((H, W), dt)
    for j in range(K):
        yy = reflect(y + j - r, H)
        for i in range(K):
            acc = acc + (w[j] * w[i]) * img[yy, reflect(x + i - r, W)]
    return acc


def smooth(field, sigma, dt=np.float64):
    """The elastic stage's Gaussian over a noise field: rows, then columns (torchvision's 2-D
    outer-product kernel up to rounding), reflect padding."""
    H, W = field.shape
    K = elastic_taps(sigma)
    r = K // 2
    assert r <= min(H, W) - 1
    w = gauss_taps(K, np.float32(sigma), dt)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = field.astype(dt)
    t = np.zeros((H, W), dt)
    for j in range(K):
        t = t + w[j] * f[y, reflect(x + j - r, W)]
    o = np.zeros((H, W), dt)
    for j in range(K):
        o = o + w[j] * t[reflect(y + j - r, H), x]
    return o


def elastic(img, alpha, sigma, nx, ny, dt=np.float64, info=None):
    """ElasticTransform(alpha, sigma) of img [H, W] given the noise fields nx, ny in [-1, 1).
    ``info`` (a dict) receives the displaced sample positions ix, iy."""
    H, W = img.shape
    img = img.astype(dt)
    alpha = dt(np.float32(alpha))
    bx, by = smooth(nx, sigma, dt), smooth(ny, sigma, dt)
    sx = (alpha * dt(W)) / (dt(2.0) * dt(H))
    sy = (alpha * dt(H)) / (dt(2.0) * dt(W))
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dx, dy = bx * sx, by * sy
    flx, fly = np.floor(dx), np.floor(dy)
    x0, y0 = x + flx.astype(np.int64), y + fly.astype(np.int64)
    lx, ly = dx - flx, dy - fly
    hx, hy = dt(1.0) - lx, dt(1.0) - ly
    if info is not None:
        info["ix"], info["iy"] = x + dx.astype(np.float64), y + dy.astype(np.float64)

    def corner(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = np.where(ok, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], dt(0))
        return v, ok.astype(dt)

    v00, m00 = corner(y0, x0)
    v01, m01 = corner(y0, x0 + 1)
    v10, m10 = corner(y0 + 1, x0)
    v11, m11 = corner(y0 + 1, x0 + 1)
    sv = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)
    mv = hy * (hx * m00 + lx * m01) + ly * (hx * m10 + lx * m11)
    return sv * mv          # img * mask + (1 - mask) * fill, fill = 0


def augment_one_x(img, rec, ext, gm, seed, rid, kinds, group=4, dt=np.float64):
    """One view through a chain with the new kinds.  Runs of old kinds go through
    oracle.augment.augment_one_seq as is (float32, bit-exact); the elastic / blur stages are
    applied in ``dt`` to what precedes them (a later run of old kinds rounds to float32 first)."""
    H, W = img.shape
    cur = np.asarray(img)
    run = []

    def flush(cur):
        if run:
            cur = OA.augment_one_seq(cur.astype(np.float32), rec, gm, seed, rid, list(run), group)
            run.clear()
        return cur

    for k in kinds:
        if k == K_BLUR:
            cur = flush(cur)
            if ext[X_SIGMA] > 0:
                cur = blur(cur, ext[X_SIGMA], int(ext[X_K]), dt)
        elif k == K_ELASTIC:
            cur = flush(cur)
            if ext[X_ALPHA] != 0:
                nx, ny = noise_fields(seed, rid, H, W)
                cur = elastic(cur, ext[X_ALPHA], ext[X_ESIGMA], nx, ny, dt)
        else:
            run.append(k)
    return flush(cur)

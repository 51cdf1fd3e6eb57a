"""The case tables of the dense GEMM family's edge tests (csrc/gemm.hip), shared by
test_gpu_gemm_edges.py (which runs them) and test_gemm_args_cpu.py (which pins their split-K
plans through the *_ws_elems entry points, so a planner change shows up on a machine without a
GPU instead of silently moving a case off the path it is there for).

Tiles and split counts are literals: they were read off plan_for once and are not recomputed
here."""


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------- avd_gemm
# (M, N, K, tile, splits, last k-chunk, modes)
ALL, MFMA = (0, 1, 2), (1, 2)
GEMM_CASES = [
    (1, 1, 1, "64x64", 1, 1, ALL),
    (3, 5, 2, "64x64", 1, 2, ALL),
    (7, 129, 64, "64x64", 1, 64, ALL),
    (65, 129, 31, "64x64", 1, 31, ALL),        # k-tile edges of both MFMA modes (BK 32 / 64)
    (65, 129, 32, "64x64", 1, 32, ALL),
    (65, 129, 33, "64x64", 1, 33, ALL),
    (65, 129, 63, "64x64", 1, 63, ALL),
    (65, 129, 64, "64x64", 1, 64, ALL),
    (65, 129, 65, "64x64", 1, 65, ALL),
    (70, 130, 45, "64x64", 1, 45, ALL),        # run with sam = 48: aligned rows, K % 4 != 0
    (132, 68, 100, "64x64", 1, 100, ALL),      # layout matrix
    (1000, 1800, 36, "128x64", 1, 36, ALL),
    (1917, 1923, 36, "128x128", 1, 36, ALL),
    (64, 64, 512, "64x64", 2, 256, ALL),
    (33, 17, 700, "64x64", 2, 316, ALL),
    (130, 70, 1001, "64x64", 3, 233, ALL),     # split + scalar staging
    (200, 100, 1100, "128x64", 4, 140, ALL),
    (256, 200, 1030, "128x128", 4, 70, ALL),   # layout matrix, split
    (5, 7, 32771, "64x64", 103, 131, ALL),     # 103 % 4 == 3: the reduce's tail loop
    (1024, 1027, 1024, "128x128", 4, 256, ALL),   # scalar reduce: 4108 blocks > its 4096 cap
    (16500, 256, 1024, "128x256", 2, 512, MFMA),  # vector reduce: 4125 blocks > the cap
    (4097, 200, 1028, "128x256", 6, 68, ALL),  # ragged N on the 256-wide tile, vector staging
    (4100, 129, 1030, "128x256", 6, 70, ALL),  # the same, scalar staging
]


def gemm_id(c):
    M, N, K, tile, S = c[:5]
    return f"{M}x{N}x{K}-{tile}" + (f"-split{S}" if S > 1 else "")


def gemm_need(c):
    """avd_gemm_ws_elems of a case in the MFMA modes."""
    M, N, _, _, S = c[:5]
    return S * M * N if S > 1 else 0


def find_gemm(M, N, K):
    return next(c for c in GEMM_CASES if c[:3] == (M, N, K))


# ---------------------------------------------------------------------------- avd_linear_bwd
# (rows, O, In, x_ld - In, path, dW splits, dX splits, avd_linear_bwd_ws_elems)
#   dW = dout^T x is the GEMM (O, In, rows), dX = dout W the GEMM (rows, In, O); the workspace
#   holds both problems' partial tiles and the bias gradient's [row chunks][O] partial sums
LINEAR_BWD_CASES = [
    (1028, 132, 136, 0, "pair dW128x128 dX64x64", 4, 1, 86988),
    (1028, 516, 136, 0, "pair both split", 4, 2, 619660),
    (2180, 132, 832, 0, "pair dX128x64", 7, 1, 784872),
    (4100, 128, 1024, 0, "pair dX128x128", 13, 1, 1719936),
    (1028, 130, 136, 0, "fallback O%4", 4, 1, 85670),
    (1028, 132, 136, 1, "fallback stride", 4, 1, 86988),
    (300, 132, 1540, 0, "fallback no 128x128 dW", 1, 1, 13200),
    (33, 24, 40, 0, "db chunk 1", 1, 1, 792),
    (127, 8, 8, 0, "db chunk 1", 1, 1, 1016),
    (129, 260, 12, 0, "db ragged chunk and strip", 1, 1, 16900),
]
# the bias gradient alone: (rows, O) over chunk 1, ragged last chunks and ragged 256-wide strips
DB_CASES = [(1, 8), (33, 256), (127, 257), (128, 260), (129, 516), (1028, 257), (1028, 516),
            (128, 8), (129, 8)]


def db_elems(rows, O):
    chunk = max(1, cdiv(rows, 128))
    return cdiv(rows, chunk) * O


def linear_bwd_id(c):
    rows, O, In, xpad, path = c[:5]
    return f"{rows}x{O}x{In}-" + path.replace(" ", "_")


# ----------------------------------------------------------------------------------- _hwc
# (rows, O, C, HW, forward splits, dW splits, dX splits, avd_linear_hwc_ws_elems)
HWC_CASES = [
    (1, 4, 8, 1, 1, 1, 1, 4),
    (7, 4, 8, 3, 1, 1, 1, 28),
    (129, 132, 24, 5, 1, 1, 1, 8580),
    (1030, 132, 24, 7, 1, 4, 1, 103884),
    (1030, 260, 64, 25, 5, 4, 1, 1693900),
    (4100, 200, 64, 16, 6, 13, 1, 4920000),
]


def hwc_id(c):
    return "x".join(str(v) for v in c[:4])

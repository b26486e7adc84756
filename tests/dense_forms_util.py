"""Which dense GEMM kernel a launch takes, and the shape lists of the GPU tests that have to reach every one of them.

nrm_gemm_nt_form (include/nrm_hotpath.h) answers, without a device, with the selector the launch itself calls.  The GPU tests
(tests/test_gpu_dense.py, tests/test_gpu_row_containment.py) take their shapes from here and assert the form with the query;
tests/test_dense_forms_cpu.py holds the set these lists reach equal to the set the selector can return, so a form added later
without a GPU case fails on any machine.  Shapes are (M, K, N): rows, reduction width, output width of the forward GEMM; the
input-gradient GEMM of the same layer is (M, N, K)."""

F32, BF16, BF16X3 = 0, 1, 2
KNOBS = ("NRM_NT_SMALLM", "NRM_NT_NARROW", "NRM_RX_BM", "NRM_RX_MIN_WGS", "NRM_GEMM_F32")


def nt_form(lib, M, N, K):
    """(NT, MT, WPE, KC) of gemm_nt_kernel<NT, MT, EPI, WPE> for y[M, N] = x[M, K] W^T in fp32; KC, the K-chunks per LDS stage, is always 1."""
    v = lib.nrm_gemm_nt_form(M, N, K, F32)
    assert v > 0, (M, N, K, v)
    return (v & 255, (v >> 8) & 255, (v >> 16) & 255, (v >> 24) & 255)


def rx_form(lib, M, N, K, mma):
    """(RT, G) of gemm_nt_rx_kernel, or None where the reduction width does not fit the resident-row form (ops then runs fp32)."""
    v = lib.nrm_gemm_nt_form(M, N, K, mma)
    assert v >= 0, (M, N, K, mma, v)
    return (v & 255, v >> 8) if v else None


def dense_form(lib, M, N, K, mma):
    """What ops._gemm_nt launches for this arithmetic: ('rx', mma, RT, G) or ('nt', NT, MT, WPE, KC)."""
    if mma != F32:
        f = rx_form(lib, M, N, K, mma)
        if f:
            return ("rx", mma) + f
    return ("nt",) + nt_form(lib, M, N, K)


def block_rows(form):
    """Rows of x one workgroup of the form holds."""
    return 16 * form[2] if form[0] == "rx" else 64 * form[2]


# ---------------------------------------------------------------------------------------------- the GPU case lists
# test_linear_forward_backward (fp32, default dispatch).  (300, 130, 128): <8,1,4>, the one-row-tile form of the 8-tile plan, which no
# other shape takes; K = 130 is nine chunks, the last one ragged
LINEAR_SHAPES = [(300, 402, 1608), (257, 1608, 402), (64, 3, 8), (1000, 402, 1), (33, 66, 64),
                 (5, 272, 68), (192, 400, 400), (700, 402, 400), (700, 400, 402), (3000, 1608, 402), (1300, 402, 1608), (300, 130, 128)]

# test_linear_forward_backward_on_bf16_matrix_cores (bf16x3 and bf16).  (51200, 64, 64) and (15360, 258, 1032): 128- and 64-row blocks.
# (25600, 128, 200): (RT, G) = (8, 4) forward; its dX (K = 200) is (8, 4) in bf16 and (4, 4) in bf16x3; 13 column tiles over 8 waves.
# (12800, 256, 40): (4, 4), three column tiles: five waves idle.  (6, 256, 40): (1, 4).
BF16_LINEAR_SHAPES = [(300, 258, 1032), (257, 1032, 258), (64, 3, 8), (1000, 402, 1), (33, 66, 64), (5, 272, 68),
                      (4099, 256, 256), (200, 1608, 402), (17, 40, 36), (51200, 64, 64), (15360, 258, 1032),
                      (25600, 128, 200), (12800, 256, 40), (6, 256, 40)]
BF16_EXPECTED = {  # (M, K, N): {mma: (forward (RT, G), dX (RT, G))}
    (25600, 128, 200): {BF16: ((8, 4), (8, 4)), BF16X3: ((8, 4), (4, 4))},
    (12800, 256, 40): {BF16: ((4, 4), (4, 3)), BF16X3: ((4, 4), (4, 3))},
    (6, 256, 40): {BF16: ((1, 4), (1, 3)), BF16X3: ((1, 4), (1, 3))},
}

# test_gemm_nt_large_grid_forms: the fp32 forms with several row tiles per wave, taken only at 512 or more workgroups.  K = 42 is
# three 16-wide chunks through the double-buffered stage loop, the last one ragged (kleft = 10, inside a lane's fragment).
LARGE_GRID_K = 42
LARGE_GRID_CASES = [  # (M, N, form)
    (131073, 64, (4, 4, 2, 1)),      # 512 full blocks of 256 rows and one block of a single row
    (65537, 160, (5, 4, 2, 1)),      # two N-chunks of five tiles
    (49153, 256, (8, 3, 2, 1)),      # last block short
    (32769, 258, (9, 2, 3, 1)),      # the second N-chunk has fewer valid tiles than NT
]
EPILOGUES = ("bias", "gelu", "dgelu", "mul")

# row containment in the forms with more than one row tile per wave / per workgroup: (arithmetic, M, K, N)
CONTAINMENT_CASES = [("f32", M, LARGE_GRID_K, N) for M, N, _ in LARGE_GRID_CASES] + [("bf16x3", 25600, 128, 200), ("bf16", 25600, 128, 200)]

MMA_BY_NAME = {"f32": F32, "bf16": BF16, "bf16x3": BF16X3}


def reached_forms(lib):
    """The set of dense_form answers over every launch the GPU cases above make (default latched knobs)."""
    out = set()
    for M, K, N in LINEAR_SHAPES:
        out |= {dense_form(lib, M, N, K, F32), dense_form(lib, M, K, N, F32)}
    for M, N, _ in LARGE_GRID_CASES:
        out.add(dense_form(lib, M, N, LARGE_GRID_K, F32))
    for mma in (BF16, BF16X3):
        for M, K, N in BF16_LINEAR_SHAPES:
            out |= {dense_form(lib, M, N, K, mma), dense_form(lib, M, K, N, mma)}
    return out

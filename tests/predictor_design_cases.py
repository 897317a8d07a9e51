"""The shapes of tests/test_gpu_predictor_design_rows.py and a pure-Python model of how the kernels of csrc/predictor_design.hip
walk them, for tests/test_predictor_design_case_table.py.  What varies with the shape:

* the downdate kernel has a lane per row and walks ranges of ROWS = 256 rows; its grid is min(ceil(n / 256), MAX_GRID), capped by
  the knob predictor_design_grid where that is positive, and workgroup w walks the ranges w, w + grid, ..; every workgroup leaves
  one partial argmax, so the grid is also the number of partials the pick kernel reduces;
* p sits in LDS for s <= LDS_S = 20480 and is gathered from global memory above;
* the projection and the initial scores add K terms over 64 lanes: K < 64 leaves lanes empty, K = 64 fills them once, K = 65 gives
  one lane a second term;
* the pick kernel has PICK = 1024 threads, a thread per k (z, v, u) and per tau (b): K or t above 1024 walk a second round;
* r runs from 1 to the ELL limit RMAX = 32: the kernels have no pair or tile edge in r (the rows are read a-major from a
  transposed copy, or in place with the knob predictor_design_pack at 0: the same entries at other addresses)."""
ROWS, MAX_GRID, PICK, LDS_S, RMAX, SMAX = 256, 1024, 1024, 20480, 32, 32768
D = 0.1                                                       # the observation variance of the kernel tests
LDP_PAD, Q = 5, 1                                             # ldp = K + q + 5, NaN from column K on

# (n, r, s, K, B): n in {1, 63, 64, 65, 257, 1000}, r in {1, 3, 10, 32}, K in {1, 15, 64, 65, 200}, B in {1, 2, K + 3, n},
# s in {r, 200, 20480, 20481} (the last two at K = 4); then K and t above the pick kernel's 1024 threads
CASES = [
    (1, 1, 1, 1, 1), (63, 3, 3, 15, 2), (64, 10, 200, 64, 64), (65, 32, 200, 65, 65), (65, 10, 200, 200, 1),
    (257, 3, 200, 200, 203), (257, 10, 200, 15, 257), (1000, 10, 200, 64, 67), (1000, 1, 200, 1, 1000), (1000, 32, 32, 15, 18),
    (257, 3, 20480, 4, 7), (257, 3, 20481, 4, 7), (1000, 10, 20480, 4, 2), (1000, 10, 20481, 4, 2),
    (63, 3, 200, 1100, 3), (1100, 1, 200, 1, 1100),
]


def ranges(n):
    return (n + ROWS - 1) // ROWS


def grid(n, knob=0):
    g = min(ranges(n), MAX_GRID)
    return min(g, knob) if knob > 0 else g


def caps(n):
    """the knob settings a shape is run under besides 0: one workgroup for everything and, with three ranges or more, an uneven
    split over two"""
    return [1] + ([2] if ranges(n) >= 3 else [])


def walk(n, r, s, K, B, knob=0):
    g = grid(n, knob)
    per = [len(range(w, ranges(n), g)) for w in range(g)]
    last = n - ROWS * (ranges(n) - 1)
    return dict(grid=g, partials=g, ranges_per_workgroup=per, p_in_lds=s <= LDS_S, ragged_wave=last % 64 != 0, last_range_rows=last,
                lane_terms=(K + 63) // 64, empty_lanes=max(0, 64 - K), uneven_lanes=K > 64 and K % 64 != 0,
                k_rounds=(K + PICK - 1) // PICK, tau_rounds=(max(B - 1, 1) + PICK - 1) // PICK, exhausted=B == n)


def workspace_bytes(n, r, s, K, B):
    """the pieces of DesignWork, each rounded up to 256 bytes"""
    up = lambda b: (b + 255) // 256 * 256
    pieces = [4 * n * r, 8 * n * r, 8 * n, n, 8 * MAX_GRID, 4 * MAX_GRID, 8, 8 * K, 8 * K, 8 * B, 8 * s, 8 * K * B, 8 * K * B]
    return sum(up(b) for b in pieces)


def shape_ok(n, r, s, K, B):
    return n >= 1 and 1 <= r <= RMAX and 1 <= s <= SMAX and K >= 1 and 1 <= B <= n

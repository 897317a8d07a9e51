"""The shapes of tests/test_gpu_predictor_gram.py and a pure-Python model of how the kernels of csrc/predictor_update.hip walk
them, for tests/test_predictor_update_case_table.py.  What varies with the shape:

* rows are cut into chunks of GC = 256 counted from row 0 of the call (grid x); a chunk is walked in steps of STEP = 32 rows of
  E in LDS, wave w of 4 building rows 8 w .. 8 w + 7 of the step, so a partial last step leaves whole waves idle and its missing
  rows are zeros that are multiplied like the others; a step is 8 MFMA k-steps of 4 rows;
* the K + q columns are cut into column tiles of CT = 64; a workgroup owns the output tile (I, J), I >= J (grid y = T (T + 1) / 2
  panels) and builds the columns of tiles I and J -- once where I = J; the last tile may be partial, and the q mean columns may
  straddle a tile edge (the residual is taken in two tiles);
* a tile is 4 x 4 blocks of 16 x 16, wave w the block row w; on a diagonal tile the blocks above the diagonal are not computed
  and the diagonal block stores its lower half; a block that lies past K + q stores nothing;
* the reduce kernel adds the chunk partials in ascending order and mirrors the lower triangle; a call of more than LAUNCH_CHUNKS
  chunks (knob predictor_gram_launch_chunks, 64; fewer where 256 MiB of partials hold fewer) is several launches whose
  reductions continue one chain in S -- the kernel tests set the knob to 1 and 2 to reach that with three chunks."""
GC, STEP, CT, WAVES, BLK = 256, 32, 64, 4, 16
LAUNCH_CHUNKS = 64

NS = [1, STEP - 1, STEP, STEP + 1, GC - 1, GC, GC + 1, 2 * GC + 3]
RS = [1, 5, 32]
SS = [1, 7, 300]
# (K, q): K + q on both sides of 16, of the column tile (= the panel width) and of two tiles; q in {1, 3}; 201 = the timed width
KQS = [(14, 1), (15, 1), (13, 3), (14, 3), (62, 1), (63, 1), (62, 3), (64, 1), (127, 3), (200, 1)]
LDP_PAD, LDS_PAD = 5, 3                                       # ldp = K + q + 5 (NaN beyond K + q), lds = K + q + 3
# the order and bound tests: one narrow and one multi-panel width, single chunk and three chunks
ORDER_CASES = [(5, 300, 14, 3, 33), (5, 300, 62, 3, GC), (32, 7, 127, 3, 2 * GC + 3), (1, 1, 15, 1, GC + 1)]


def walk(n, K, q):
    W = K + q
    chunks = (n + GC - 1) // GC
    last_chunk = n - GC * (chunks - 1)
    steps = (last_chunk + STEP - 1) // STEP
    last_step = last_chunk - STEP * (steps - 1)
    per_wave = STEP // WAVES
    T = (W + CT - 1) // CT
    last_cols = W - CT * (T - 1)
    return dict(chunks=chunks, last_chunk_rows=last_chunk, steps_in_last_chunk=steps, last_step_rows=last_step,
                partial_step=last_step < STEP, idle_waves=WAVES - (last_step + per_wave - 1) // per_wave,
                zero_k_steps=(STEP - last_step) // 4, ragged_k_step=last_step % 4 != 0,
                tiles=T, panels=T * (T + 1) // 2, last_tile_cols=last_cols, partial_tile=last_cols < CT,
                partial_block=W % BLK != 0, empty_blocks_in_last_tile=(CT - last_cols) // BLK,
                mean_straddles_a_tile=q > 1 and K // CT != (W - 1) // CT, mean_tile=K // CT, q=q)


def panel_of(p):
    """(I, J) of grid row p, as the kernel finds it"""
    I, J = 0, p
    while J > I:
        J -= I + 1
        I += 1
    return I, J


def blocks_of(I, J, wave):
    """the block columns wave `wave` multiplies on tile (I, J)"""
    return list(range(wave + 1 if I == J else CT // BLK))


def launch_chunks(K, q, knob=LAUNCH_CHUNKS):
    """the chunks of one launch: the knob (at least 1), no more than 256 MiB of partials hold"""
    return min(max(1, knob), max(1, (256 << 20) // (8 * (K + q) ** 2)))


def launches(n, K, q, knob=LAUNCH_CHUNKS):
    per = launch_chunks(K, q, knob)
    return ((n + GC - 1) // GC + per - 1) // per


def workspace_bytes(n, K, q, knob=LAUNCH_CHUNKS):
    return 8 * (K + q) ** 2 * min((n + GC - 1) // GC, launch_chunks(K, q, knob))


def update_block(extend_block):
    """the rows per block of flgp_predictor_update: model_extend_block (at least 256) rounded down to a multiple of GC, at least GC"""
    return max(GC, max(256, extend_block) // GC * GC)

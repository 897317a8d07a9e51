"""The shapes of tests/test_gpu_nystrom_predictor_rows.py and a pure-Python model of how flgp_dev_nystrom_predictor_rows
(csrc/nystrom_predictor.hip) walks them, for tests/test_nystrom_predictor_case_table.py.  What varies with the shape:

* the anchor chunks (blockIdx.y): ceil(s / 64) chunks of 64 anchors, the last one full or partial;
* the workgroups of 256 rows (blockIdx.x) and the rows of the last one; the finishing kernel's workgroups of 64 rows;
* the dot-product route: the register kernel np_sim_kernel<DP> for dpad = 4, 8, 16, 32, 64, or the GEMM's dot products and
  np_exp_rows_kernel (d > 32 by default, knob nystrom_dot_gemm; always for d > 64);
* the passes of CM = 8 mean columns over groups q columns, the columns of the last pass, and what the first pass does with Z
  (register route: stored only for a variance; GEMM route: v written back for a variance or a further pass);
* the variance: groups per chunk of T under the cap nystrom_predictor_t_mb, and the chunks."""
CM = 8
BASE = dict(n=257, d=9, s=130, K=65, q=1, groups=1)
S_VALUES = [1, 63, 64, 65, 130, 257]
N_VALUES = [1, 255, 256, 257, 513]
D_VALUES = [1, 3, 5, 9, 17, 33, 64, 70]
K_VALUES = [1, 63, 64, 65, 130]
QG_VALUES = [(1, 1), (3, 1), (1, 3), (3, 3), (1, CM), (1, CM + 1)]          # (q, groups): groups q = 1, 3, 3, 9, CM, CM + 1
OUTPUTS = [(True, True), (True, False), (False, True)]                    # (mean, var)
BIT_ROWS = 513                                                            # the bit checks: 513 rows, K = 130, three groups
T_MB_SMALL = 1                                                            # the cap at which those groups go one at a time


def cases():
    """one dimension at a time around BASE; every value of every list appears"""
    out = []
    for key, values in (("s", S_VALUES), ("n", N_VALUES), ("d", D_VALUES), ("K", K_VALUES)):
        for v in values:
            c = dict(BASE, **{key: v})
            if c not in out:
                out.append(c)
    for q, groups in QG_VALUES:
        c = dict(BASE, q=q, groups=groups)
        if c not in out:
            out.append(c)
    out.append(dict(BASE, d=40, q=3, groups=3))      # the GEMM route with two passes: v is written back without a variance
    out.append(dict(BASE, d=70, s=65, n=513))        # d > 64 with more than one workgroup and a one-anchor last chunk
    return out


def dpad(d):
    for p in (4, 8, 16, 32, 64):
        if d <= p:
            return p
    return (d + 7) // 8 * 8


def route(d, dot_gemm=-1):
    p = dpad(d)
    return "gemm" if p > 64 or dot_gemm == 1 or (dot_gemm < 0 and p > 32) else "reg%d" % p


def walk(n, d, s, K, q, groups, mean=True, var=True, dot_gemm=-1, t_mb=256):
    gq = groups * q if mean else 0
    npass = -(-gq // CM)
    r = route(d, dot_gemm)
    if r == "gemm":
        first = "written back" if (var or npass > 1) else "left as dots"
    else:
        first = "stored" if var else "not stored"
    gc = max(1, min(groups, (t_mb << 20) // (8 * n * (K + q)))) if var else 0
    return dict(chunks=-(-s // 64), tail=s - 64 * (-(-s // 64) - 1), blocks=-(-n // 256), last_block_rows=n - 256 * (-(-n // 256) - 1),
                finish_blocks=-(-n // 64), route=r, passes=npass, last_pass_cols=gq - CM * (npass - 1) if npass else 0, z=first,
                groups_per_t=gc, t_chunks=-(-groups // gc) if var else 0)

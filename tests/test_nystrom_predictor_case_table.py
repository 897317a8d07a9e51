"""CPU: the case list of tests/test_gpu_nystrom_predictor_rows.py holds every value the issue names and reaches every way
flgp_dev_nystrom_predictor_rows walks a shape, by the pure-Python model of tests/nystrom_predictor_cases.py; the model's
constants are those of csrc/nystrom_predictor.hip."""
import os
import re

import nystrom_predictor_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _walks(**kw):
    return [nc.walk(**c, **kw) for c in nc.cases()]


def test_the_model_has_the_sources_constants():
    src = open(os.path.join(ROOT, "flgp_amd", "csrc", "nystrom_predictor.hip")).read()
    assert int(re.search(r"constexpr int NP_CM = (\d+);", src).group(1)) == nc.CM
    assert re.search(r'tuning\("nystrom_predictor_t_mb", 256\)', src)
    assert "blockIdx.x * 256 + threadIdx.x" in src and "blockIdx.y * 64" in src and "blockIdx.x * 64 + threadIdx.x" in src


def test_every_named_value_is_in_the_list():
    cs = nc.cases()
    for key, values in (("s", [1, 63, 64, 65, 130, 257]), ("n", [1, 255, 256, 257, 513]), ("d", [1, 3, 5, 9, 17, 33, 64, 70]),
                        ("K", [1, 63, 64, 65, 130]), ("q", [1, 3]), ("groups", [1, 3])):
        assert {c[key] for c in cs} >= set(values), key
    assert {c["groups"] * c["q"] for c in cs} >= {nc.CM, nc.CM + 1}
    assert nc.OUTPUTS == [(True, True), (True, False), (False, True)]
    assert len(cs) == len({tuple(sorted(c.items())) for c in cs}) and len(cs) <= 32


def test_chunk_workgroup_and_route_edges():
    w = _walks()
    assert {x["chunks"] for x in w} >= {1, 2, 3, 5}
    assert {x["tail"] for x in w} >= {1, 2, 63, 64}                       # a one-anchor, a partial and a full last chunk
    assert {x["blocks"] for x in w} == {1, 2, 3}
    assert {x["last_block_rows"] for x in w} >= {1, 255, 256}             # a lone row, a partial and a full last workgroup
    assert {x["finish_blocks"] for x in w} >= {1, 4, 5, 9}
    assert {x["route"] for x in w} == {"reg4", "reg8", "reg16", "reg32", "gemm"}      # d = 33 .. 64 go to the GEMM by default,
    assert {x["route"] for x in _walks(dot_gemm=0)} == {"reg4", "reg8", "reg16", "reg32", "reg64", "gemm"}   # reg64 with the knob
    assert nc.route(70, 0) == "gemm" and nc.route(64, 0) == "reg64" and nc.route(9, 1) == "gemm"


def test_pass_and_z_edges():
    both, mean_only, var_only = (_walks(mean=m, var=v) for m, v in nc.OUTPUTS)
    assert {x["passes"] for x in both} == {1, 2} and {x["passes"] for x in var_only} == {0}
    assert {x["last_pass_cols"] for x in both} >= {1, 3, nc.CM}           # CM: a full single pass; CM + 1: a second pass of one
    assert nc.walk(**dict(nc.BASE, groups=nc.CM + 1))["last_pass_cols"] == 1
    assert {x["z"] for x in mean_only} == {"not stored", "left as dots", "written back"}
    assert {x["z"] for x in both} == {"stored", "written back"} == {x["z"] for x in var_only}
    # the GEMM route writes v back without a variance only for a further pass
    assert nc.walk(**dict(nc.BASE, d=40, q=3, groups=3), var=False)["z"] == "written back"
    assert nc.walk(**dict(nc.BASE, d=40), var=False)["z"] == "left as dots"


def test_the_bit_check_reaches_the_t_chunks():
    shape = dict(nc.BASE, n=nc.BIT_ROWS, K=130, q=1, groups=3)
    assert nc.walk(**shape)["t_chunks"] == 1 and nc.walk(**shape)["groups_per_t"] == 3
    small = nc.walk(**shape, t_mb=nc.T_MB_SMALL)
    assert small["groups_per_t"] == 1 and small["t_chunks"] == 3

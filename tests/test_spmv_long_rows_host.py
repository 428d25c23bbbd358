"""What the long-row path of A.w / B.w adds on the host side (no GPU): the four fields zk_prover_info reports, laid out in
lib.py as in include/zkhip.h, and the --long-rows option of tools/zkgen.py."""
import ctypes as C
import importlib.util
import os
import subprocess

import pytest

from conftest import ROOT

FIELDS = ["spmv_row_cut", "spmv_long_rows", "spmv_longest_row", "spmv_chunks"]


def test_prover_plan_layout_matches_the_header(tmp_path):
    from rapidsnark_old_amd import lib as L
    names = [n for n, _ in L.zk_prover_plan._fields_]
    assert names[-4:] == FIELDS                                     # appended: the struct is size-versioned
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zkhip.h"\nint main(void) {\n    printf("%zu", sizeof(zk_prover_plan));\n'
                   + "".join('    printf(" %%zu", offsetof(zk_prover_plan, %s));\n' % f for f in FIELDS) + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(L.zk_prover_plan)] + [getattr(L.zk_prover_plan, f).offset for f in FIELDS]
    assert all(getattr(L.zk_prover_plan, f).size == 4 for f in FIELDS)


def _cli():
    spec = importlib.util.spec_from_file_location("zkgen_cli", os.path.join(ROOT, "tools", "zkgen.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_zkgen_cli_long_rows_option(capsys):
    cli = _cli()
    assert cli.parse_args(["10", "out"]).long_rows == []
    assert cli.parse_args(["10", "out", "--long-rows", "3x254"]).long_rows == [(3, 254)]
    args = cli.parse_args(["10", "out", "--circuit-like", "--long-rows", "3x254", "--long-rows", "1X5000"])
    assert args.long_rows == [(3, 254), (1, 5000)] and args.circuit_like
    # 2^4 domain, 2 public signals: 3 input signals, 12 constraints -> 24 picks fit, 25 do not
    assert cli.parse_args(["4", "out", "--long-rows", "24x5"]).long_rows == [(24, 5)]
    for bad in (["--long-rows", "0x5"], ["--long-rows", "3x0"], ["--long-rows", "3"], ["--long-rows", "ax5"], ["--long-rows", "-1x5"],
                ["--long-rows", "25x5"], ["--long-rows", "20x5", "--long-rows", "5x9"], ["--semaphore-like", "--long-rows", "1x5"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["4", "out"] + bad)
        assert e.value.code == 2, bad
    capsys.readouterr()


def test_zkgen_long_rows_are_checked_before_any_gpu_work():
    from rapidsnark_old_amd import zkgen
    assert zkgen.constraint_count(10, 2) == (1024 - 1 - 128, 128)
    assert zkgen.constraint_count(10, 2, circuit_like=True) == (768 + 5 - 1 - 128, 128)
    assert zkgen.check_long_rows([(1, 5000), (4, 300)], 895) == [(1, 5000), (4, 300)]
    assert zkgen.check_long_rows((), 1) == []
    for bad in ([(0, 5)], [(3, 0)], [(3, 5)]):
        with pytest.raises(ValueError):
            zkgen.check_long_rows(bad, 1)

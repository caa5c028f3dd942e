"""The SOP engine's arithmetic cores as the device compiler builds them, against exact integers: the final reduction
sop_reduce (csrc/lcv_sop.hpp: an FP64 quotient estimate whose conditional subtraction real data takes about once in
2^29 ops), the Montgomery product / square fp_mul_c28 / fp_sqr_c28 and the column products and reduction sop_mac28 /
sop_kara_mac / sop_kara_join / sop_redc28 (csrc/lcv_col28.hpp).  build/soptest (tools/microbench/soptest.hip, built
by `make all`) runs one case per lane and only moves data; every case of sop_vectors.py is judged here with Python
integers, by the same check_* functions as on the CPU twins (test_sop_reduce_cpu.py, test_col28_cpu.py,
test_sop_arith_cpu.py): on and around every multiple of p and the skip threshold of the reduction, lazily reduced
operands and saturated / sparse limb patterns, and for every op shape of the generated programs the operands that
bring a 64-bit column closest to overflow."""
import os
import subprocess

import pytest

import sop_vectors as V

pytestmark = pytest.mark.gpu

BUILD = os.path.join(os.path.dirname(__file__), "..", "light-client-consensus-specs_amd", "build")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One run of build/soptest over all three sections."""
    exe = os.path.join(BUILD, "soptest")
    if not os.path.exists(exe):
        return {"exe": exe, "proc": None}
    d = tmp_path_factory.mktemp("soptest")
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    red, c28, cols = V.reduce_cases(), V.c28_cases(), V.column_cases()
    with open(fin, "wb") as f:
        f.write(V.pack_input(red, c28, cols))
    proc = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=90)
    out = None
    if proc.returncode == 0:
        with open(fout, "rb") as f:
            out = V.unpack_output(f.read(), len(red), len(c28), len(cols))
    return {"exe": exe, "proc": proc, "out": out}


def _section(run, k):
    assert run["proc"] is not None, f"{run['exe']} missing: run make all"
    assert run["proc"].returncode == 0, run["proc"].stdout + run["proc"].stderr
    return run["out"][k]


def test_reduce_exact(run):
    cases, got = V.reduce_cases(), _section(run, 0)
    assert len(got) == len(cases) > 20000
    for case, words in zip(cases, got):
        V.check_reduce(case, words)


def test_c28_exact(run):
    cases, got = V.c28_cases(), _section(run, 1)
    assert len(got) == len(cases) >= 3 * 91
    for case, (mul, sqr) in zip(cases, got):
        V.check_c28(case, mul, sqr)


def test_columns_exact(run):
    cases, got = V.column_cases(), _section(run, 2)
    assert len(got) == len(cases) >= 900
    for case, (cols, words) in zip(cases, got):
        V.check_columns(case, cols, words)

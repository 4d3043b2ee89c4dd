"""CPU check of the chain objective's host-side table builders (kaldi-fp16_amd/csrc/chain_tables.cpp).

Every numerical property of the denominator follows from these tables: the per-row summation
order, the placement of records within a slice step, tp = 0 padding records on valid indices,
each slice owned by exactly one (block, wave). chain_tables.cpp includes no HIP header, so
tests/chain_tables/check_main.cpp links it alone into a stand-alone program that checks those
properties from the input arcs (not against a digest of the builders' output) on small graphs,
and prints one line per check. The program is built twice, plain and under AddressSanitizer and
UBSan with the runtimes linked statically; nothing is loaded into Python.
"""
import concurrent.futures
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kaldi-fp16_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SOURCES = [os.path.join(CSRC, "chain_tables.cpp"), os.path.join(ROOT, "tests", "chain_tables", "check_main.cpp")]

# the sanitizer runtimes are linked statically, so the program runs in any inherited environment
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SAN_GXX = SAN + ["-static-libasan", "-static-libubsan"]
SAN_CLANG = SAN + ["-static-libsan"]

GRAPHS = ["S1", "S31", "S33", "S64", "S65", "S129", "skew", "deadends", "P33", "P4096"]
TABLE_CHECKS = ["perm", "len_off", "records", "padding", "positions", "scaled"]
EXPECTED = set()
for _g in GRAPHS:
    EXPECTED |= {(_g, "accepted"), (_g, "ownership")}
    EXPECTED |= {("%s.%s" % (_g, t), c) for t in "fbq" for c in TABLE_CHECKS}
EXPECTED |= {("balance.nsl%d.G%d" % (n, g), "slots") for n in (1, 15, 16, 17, 111) for g in (1, 2, 4, 8)}
EXPECTED |= {("num." + f, "prepared") for f in ("one_state", "chain", "lattice")}
EXPECTED |= {("num.pack", "tiles"), ("initial_probs.two_state", "closed_form"), ("initial_probs.dead_end", "finite")}

# the text each malformed input is refused with
REFUSED = {
    "num.row_ptr_not_monotone": "row_ptr not monotone",
    "num.destination_out_of_range": "arc destination out of range",
    "num.final_out_of_range": "final state out of range",
    "num.row_ptr_end": "row_ptr does not describe num_arcs arcs",
    "den.S65536": "den graph needs num_states, num_pdfs <= 65535 (16-bit arc fields)",
    "den.P4097": "num_pdfs > 4096 not supported",
    "den.negative_tp": "den transition out of range (state, pdf or negative probability)",
    "den.nan_tp": "den transition out of range (state, pdf or negative probability)",
}


def _build(outdir, name, compilers):
    """compilers: (compiler, extra flags) pairs, tried in turn"""
    exe = os.path.join(outdir, name)
    errs = []
    for cxx, extra in compilers:
        cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-I" + CSRC] + extra + SOURCES + ["-o", exe]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True)
        except FileNotFoundError as e:
            errs.append(str(e))
            continue
        if r.returncode == 0:
            return exe
        errs.append(r.stderr[-4000:])
    raise AssertionError("building %s failed:\n%s" % (name, "\n".join(errs)))


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, "%s exited %d\n%s\n%s" % (exe, r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """Builds and runs the plain and the sanitized program side by side: tag -> text or the failure."""
    outdir = str(tmp_path_factory.mktemp("chain_tables"))

    def one(job):
        tag, compilers = job
        try:
            return tag, _run(_build(outdir, "chain_tables_" + tag, compilers))
        except AssertionError as e:
            return tag, e

    jobs = [("plain", [("g++", [])]),
            ("san", [("g++", SAN_GXX), (os.path.join(ROCM, "llvm", "bin", "clang++"), SAN_CLANG)])]
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        return dict(ex.map(one, jobs))


def _check(outputs, tag):
    text = outputs[tag]
    if isinstance(text, AssertionError):
        raise text
    lines = text.splitlines()
    failed = [ln for ln in lines if ln.startswith("FAIL ")]
    assert not failed, "\n".join(failed)
    assert lines[-1] == "DONE 0 failure(s)", lines[-1]
    passed = [tuple(ln.split()[1:]) for ln in lines if ln.startswith("PASS ")]
    assert len(passed) == len(set(passed)), "a check was printed twice"
    assert set(passed) == EXPECTED, "missing %s, unexpected %s" % (
        sorted(EXPECTED - set(passed)), sorted(set(passed) - EXPECTED))
    refused = dict(ln[len("REFUSED "):].split(": ", 1) for ln in lines if ln.startswith("REFUSED "))
    assert refused == REFUSED
    assert len(lines) == len(passed) + len(refused) + 1, "lines that are no finding"


def test_chain_tables_properties(outputs):
    _check(outputs, "plain")


def test_chain_tables_sanitized(outputs):
    """The same program under AddressSanitizer and UBSan: it runs clean (a report ends the run
    with a non-zero status) and finds the same."""
    _check(outputs, "san")

"""CPU launch trace of the host layer (kaldi-fp16_amd/host).

The host layer is pure orchestration: its behaviour is the ordered sequence of C-ABI calls it
makes into libkaldi_fp16 and their arguments. tests/host_trace/stub_backend.cpp defines every
such symbol as a function that prints one line; tests/host_trace/trace_main.cpp drives nnet_*
through the scenarios (every config, stream placements, row sets at every residue of
(T - 1) % 3, fp8, implicit dz, the debug hooks, the Kaldi-style update, the orthonormal
constraint, natural gradient, dropout, SpecAugment, training-mode BatchNorm, every pair of
modes that cannot be combined, negative cases). Each scenario's SHA-256 and
line count (and a short digest of every line) are pinned in tests/golden/host_trace.json,
so a refactor of the host layer that moves, drops or changes one launch, argument, stream, event, allocation or error text fails
here, without a GPU.

The golden is regenerated (only when a change of the launch sequence is intended) with
    HOST_TRACE_UPDATE=1 pytest tests/test_host_trace.py
"""
import base64
import concurrent.futures
import glob
import hashlib
import json
import os
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kaldi-fp16_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_trace.json")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _sources():
    # the sources of libkaldi_fp16_nnet.so (the egs reader is a library of its own)
    host = sorted(p for p in glob.glob(os.path.join(PKG, "host", "*.cpp")) if os.path.basename(p) != "egs.cpp")
    return host + [os.path.join(PKG, "csrc", "dp.cpp"),
                   os.path.join(ROOT, "tests", "host_trace", "stub_backend.cpp"),
                   os.path.join(ROOT, "tests", "host_trace", "trace_main.cpp")]


def _build(outdir, name, compilers):
    """compilers: (compiler, extra flags) pairs, tried in turn"""
    exe = os.path.join(outdir, name)
    errs = []
    for cxx, extra in compilers:
        flags = ["-std=c++17", "-g", "-O1", "-Wall", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__",
                 "-I" + os.path.join(ROCM, "include")] + extra
        objs = [os.path.join(outdir, "%s_%d.o" % (name, i)) for i in range(len(_sources()))]
        try:  # one compiler process per source, side by side
            procs = [subprocess.Popen([cxx] + flags + ["-c", src, "-o", obj], stderr=subprocess.PIPE, text=True)
                     for src, obj in zip(_sources(), objs)]
        except FileNotFoundError as e:
            errs.append(str(e))
            continue
        out = [p.communicate()[1] for p in procs]
        if any(p.returncode for p in procs):
            errs.append("".join(out)[-4000:])
            continue
        r = subprocess.run([cxx] + extra + objs + ["-o", exe, "-ldl"], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errs.append(r.stderr[-4000:])
    raise AssertionError("building %s failed:\n%s" % (name, "\n".join(errs)))


def _run(exe):
    r = subprocess.run([exe, os.path.join(ROOT, "configs")], capture_output=True, text=True)
    assert r.returncode == 0, "%s exited %d\n%s" % (exe, r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    return r.stdout


def _split(text):
    scen, name = {}, None
    for ln in text.splitlines():
        if ln.startswith("== scenario "):
            name = ln[len("== scenario "):]
            assert name not in scen, "scenario printed twice: " + name
            scen[name] = []
        else:
            assert name is not None, "output before the first scenario: " + ln
            scen[name].append(ln)
    return scen


def _line_digests(lines):
    # three hex digits of every line's own digest: they name the first differing line
    return "".join(hashlib.sha256(ln.encode()).hexdigest()[:3] for ln in lines)


def _digest(scen):
    """The golden's content: per scenario [SHA-256 of the trace, line count], and the line
    digests of all scenarios (sorted by name, one after the other; the scenarios repeat each
    other a lot) deflated into one base64 string."""
    blob = "".join(_line_digests(scen[k]) for k in sorted(scen)).encode()
    z = base64.b64encode(zlib.compress(blob, 9)).decode()
    return {"scenarios": {k: [hashlib.sha256("\n".join(v).encode()).hexdigest(), len(v)] for k, v in scen.items()},
            "line_digests": [z[i:i + 2000] for i in range(0, len(z), 2000)]}


def _write_golden(d):
    with open(GOLDEN, "w") as f:  # one scenario per line
        f.write('{"scenarios": {\n')
        f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(d["scenarios"].items())))
        f.write('\n},\n"line_digests": [\n')
        f.write(",\n".join(" " + json.dumps(x) for x in d["line_digests"]))
        f.write("\n]}\n")


def _check(text, outdir, tag):
    scen = _split(text)
    got = _digest(scen)["scenarios"]
    with open(GOLDEN) as f:
        golden = json.load(f)
    want = golden["scenarios"]
    blob = zlib.decompress(base64.b64decode("".join(golden["line_digests"]))).decode()
    assert len(blob) == 3 * sum(v[1] for v in want.values()), "the golden's line digests do not match its line counts"
    bad = [k for k in sorted(want) if got.get(k) != want[k]] + [k for k in sorted(got) if k not in want]
    if not bad:
        return
    path = os.path.join(outdir, "host_trace_%s.txt" % tag)
    with open(path, "w") as f:
        f.write(text)
    msg = "%d scenario(s) differ from %s (%s); the trace is in %s" % (len(bad), GOLDEN, ", ".join(bad[:6]), path)
    k = bad[0]
    if k in got and k in want:
        at = 3 * sum(want[j][1] for j in sorted(want) if j < k)
        a, b = blob[at:at + 3 * want[k][1]], _line_digests(scen[k])
        i = next((i for i in range(0, min(len(a), len(b)), 3) if a[i:i + 3] != b[i:i + 3]), min(len(a), len(b))) // 3
        msg += "\nscenario %s: %d calls (golden %d), first differing line %d of the scenario: %s" % (
            k, got[k][1], want[k][1], i + 1, scen[k][i] if i < len(scen[k]) else "(end of trace)")
    else:
        msg += "\nscenario %s is %s" % (k, "not in the golden" if k in got else "missing from the trace")
    raise AssertionError(msg)


# the sanitizer runtimes are linked statically, so the program runs in any inherited environment
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SAN_GXX = SAN + ["-static-libasan", "-static-libubsan"]
SAN_CLANG = SAN + ["-static-libsan"]


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    """Builds and runs the plain and the sanitized program side by side: tag -> text or the failure."""
    outdir = str(tmp_path_factory.mktemp("host_trace"))

    def one(job):
        tag, compilers = job
        try:
            return tag, _run(_build(outdir, "host_trace_" + tag, compilers))
        except AssertionError as e:
            return tag, e

    jobs = [("plain", [("g++", [])]),
            ("san", [("g++", SAN_GXX), (os.path.join(ROCM, "llvm", "bin", "clang++"), SAN_CLANG)])]
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        return outdir, dict(ex.map(one, jobs))


def _text(traces, tag):
    if isinstance(traces[1][tag], AssertionError):
        raise traces[1][tag]
    return traces[1][tag]


def test_host_trace_matches_golden(traces):
    text = _text(traces, "plain")
    if os.environ.get("HOST_TRACE_UPDATE") == "1":
        _write_golden(_digest(_split(text)))
    _check(text, traces[0], "plain")


def test_dropout_switched_off_is_the_plain_trace(traces):
    """With the dropout switch off the host layer makes the calls it makes when the switch was
    never touched: the two scenarios differ by the set_dropout status line alone."""
    scen = _split(_text(traces, "plain"))
    off = [ln for ln in scen["dropout/off"] if not ln.startswith("-- set_dropout ")]
    assert len(off) == len(scen["dropout/off"]) - 1
    assert off == scen["dropout/plain"]


def test_host_trace_sanitized(traces):
    """The same stand-alone program under AddressSanitizer and UBSan: it runs clean (a report
    ends the run with a non-zero status) and gives the same digests."""
    _check(_text(traces, "san"), traces[0], "san")

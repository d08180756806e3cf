"""The proxy-side device surface on the GPU, bit for bit against the plain model of
proxy_primitive_cases: tests/bin/test_proxy_primitives (tests/cpp/test_proxy_primitives.hip, written in
the reference's spellings and compiled against include/) runs the whole case table in ONE process and
dumps, per case, the raw ring, head / tail / tailCache, the returned positions, the semaphore words, the
arenas and the error record; these tests judge the dump.  Groups T (trigger images) and F (positions,
laps, poll) run on hand-built handles with no consumer; groups P and R go through this library's own
proxy in loopback.  The same source compiled against the reference's own headers
(oracle/_ref/test_proxy_primitives_ref, oracle/build_ref.sh) is the second judge of groups T and F:
its rings, positions, head and tailCache must equal this library's byte for byte.  There is no
tolerance anywhere, no retry, and once a program has failed nothing further is launched from here."""
import os
import subprocess
import time

import pytest

import proxy_primitive_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "bin", "test_proxy_primitives")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "test_proxy_primitives_ref")

_failed = []  # the first program failure of this module; nothing is launched after it


def _run(exe, case_file, out_file):
    if _failed:
        pytest.fail("not launched: " + _failed[0], pytrace=False)
    t0 = time.time()
    env = dict(os.environ, MSCCLPP_AMD_SPIN_TIMEOUT_MS="3000")
    try:
        r = subprocess.run([exe, case_file, out_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           timeout=120, env=env)
        code, err = r.returncode, r.stderr
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        code = "killed by its time limit"
    if code != 0:
        _failed.append(f"{os.path.basename(exe)} ended with {code}:\n{err[-3000:]}")
        pytest.fail(_failed[0], pytrace=False)
    with open(out_file, "rb") as f:
        out = C.parse_output(f.read())
    print(f"{os.path.basename(exe)}: {len(out)} cases in {time.time() - t0:.2f} s")
    return out


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("proxy_primitives")
    paths = str(d / "cases.txt"), str(d / "cases_ref.txt")
    C.write_case_file(paths[0])
    C.write_case_file(paths[1], for_reference=True)
    return d, paths


@pytest.fixture(scope="module")
def lib_run(built, case_files):
    d, (all_cases, _) = case_files
    out = _run(EXE, all_cases, str(d / "out.bin"))
    assert sorted(out) == [c.idx for c in C.CASES]
    return out


@pytest.fixture(scope="module")
def ref_run(built, case_files, lib_run):
    if not os.path.exists(REF_EXE):
        pytest.skip("oracle/_ref/test_proxy_primitives_ref not built (needs /root/reference at build time)")
    d, (_, ref_cases) = case_files
    out = _run(REF_EXE, ref_cases, str(d / "out_ref.bin"))
    assert sorted(out) == [c.idx for c in C.CASES if c.ref]
    return out


def _key(c):
    if c.group == "F" and c.op == "push":
        return (c.group, "push-" + c.tag.split("-")[0], 0)  # sequential laps / many lanes
    return (c.group, c.op, C.member(c).bound if c.op in C.MEMBER_OPS else 0)


def _variants():
    seen = []
    for c in C.CASES:
        if _key(c) not in seen:
            seen.append(_key(c))
    return seen


VARIANTS = _variants()


def _id(key):
    group, op, bound = key
    return f"{group}-{op}" + ("-bound" if bound else "")


def _judge(run, key, only_ref=False):
    failures, n = [], 0
    for c in C.CASES:
        if _key(c) != key or (only_ref and not c.ref):
            continue
        n += 1
        got = run[c.idx]
        msg = C.judge_member(c, got) if c.op in C.MEMBER_OPS else C.judge_proxy(c, got)
        if msg:
            failures.append(f"{msg}; {C.describe(c)}")
    assert not failures, f"{len(failures)} of {n} cases differ; first:\n" + "\n".join(failures[:5])
    return n


@pytest.mark.parametrize("key", VARIANTS, ids=_id)
def test_proxy_primitive_matches_model(lib_run, key):
    assert _judge(lib_run, key) > 0


REF_VARIANTS = [k for k in VARIANTS if any(c.ref for c in C.CASES if _key(c) == k)]


@pytest.mark.parametrize("key", REF_VARIANTS, ids=_id)
def test_reference_headers_match_model_and_library(lib_run, ref_run, key):
    """The same source against the reference's include tree, no consumer at all: its dump equals the
    model's and, where the order of concurrent pushers is not free, this library's byte for byte."""
    assert _judge(ref_run, key, only_ref=True) > 0
    for c in C.CASES:
        if _key(c) != key or not c.ref:
            continue
        lib, ref = lib_run[c.idx], ref_run[c.idx]
        for k in ("head", "tail", "tailCache"):
            assert lib[k] == ref[k], f"{k}: library {lib[k]}, reference {ref[k]}; {C.describe(c)}"
        if C.member(c).active == 1:
            assert lib["pos"] == ref["pos"], C.describe(c)
            assert lib["ring"].tobytes() == ref["ring"].tobytes(), C.describe(c)
        else:  # which lane gets which position is free; the slots' contents as a set are not
            assert sorted(lib["pos"]) == sorted(ref["pos"]), C.describe(c)
            assert sorted(map(tuple, lib["ring"].tolist())) == sorted(map(tuple, ref["ring"].tolist())), C.describe(c)

"""The device primitive surface on the GPU, bit for bit against the plain model of
device_primitive_cases: tests/bin/test_device_primitives (tests/cpp/test_device_primitives.hip, written
in the reference's spellings and compiled against include/) runs the whole case table in ONE process,
dumps the three arenas and the error record of every case, and these tests judge the dump -- copy /
put / get at every <Alignment, CopyRemainder>, the LL16 / LL8 packet forms, the packet classes,
read<T> / write<T> and the semaphore handles.  The same source compiled against the reference's own
headers (oracle/_ref/test_device_primitives_ref, oracle/build_ref.sh) is the second judge: its arenas
must equal the model's and this library's byte for byte.  There is no tolerance anywhere."""
import os
import subprocess
import time

import pytest

import device_primitive_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "bin", "test_device_primitives")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "test_device_primitives_ref")


def _run(exe, case_file, out_file):
    t0 = time.time()
    r = subprocess.run([exe, case_file, out_file], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    with open(out_file, "rb") as f:
        bases, out = C.parse_output(f.read())
    print(f"{os.path.basename(exe)}: {len(out)} cases in {time.time() - t0:.2f} s")
    return bases, out


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_primitives")
    paths = str(d / "cases.txt"), str(d / "cases_ref.txt")
    C.write_case_file(paths[0])
    C.write_case_file(paths[1], for_reference=True)
    return d, paths


@pytest.fixture(scope="module")
def lib_run(built, case_files):
    d, (all_cases, _) = case_files
    bases, out = _run(EXE, all_cases, str(d / "out.bin"))
    assert sorted(out) == [c.idx for c in C.CASES]
    return bases, out


@pytest.fixture(scope="module")
def ref_run(built, case_files):
    if not os.path.exists(REF_EXE):
        pytest.skip("oracle/_ref/test_device_primitives_ref not built (needs /root/reference at build time)")
    d, (_, ref_cases) = case_files
    bases, out = _run(REF_EXE, ref_cases, str(d / "out_ref.bin"))
    assert sorted(out) == [c.idx for c in C.CASES if c.ref]
    return bases, out


def _variants():
    seen = []
    for c in C.CASES:
        key = (c.group, c.op, c.p0, c.p1)
        if key not in seen:
            seen.append(key)
    return seen


VARIANTS = _variants()


def _id(key):
    group, op, p0, p1 = key
    if group == "A":
        return f"A-{op}<{p0},{'true' if p1 else 'false'}>"
    if group == "D":
        return f"D-{'channel' if p1 else 'free'}-{C.RW_TYPES[p0]}"
    if group == "E":
        return f"E-{op}"
    return f"{group}-{op}-LL{p0}"


def _judge(run, key, only_ref=False):
    bases, out = run
    failures, n = [], 0
    for c in C.CASES:
        if (c.group, c.op, c.p0, c.p1) != key or (only_ref and not c.ref):
            continue
        n += 1
        err, arenas = out[c.idx]
        msg = C.first_difference(c, arenas, C.expected(c, bases=bases), bases)
        if msg:
            failures.append(msg)
        if err != [0, 0, 0, 0]:
            failures.append(f"error record {[hex(x) for x in err]}; case: {C.format_case(c)}")
    assert not failures, f"{len(failures)} of {n} cases differ; first:\n" + "\n".join(failures[:5])
    return n


@pytest.mark.parametrize("key", VARIANTS, ids=_id)
def test_primitive_matches_model(lib_run, key):
    assert _judge(lib_run, key) > 0


REF_VARIANTS = [k for k in VARIANTS if any(c.ref for c in C.CASES if (c.group, c.op, c.p0, c.p1) == k)]


@pytest.mark.parametrize("key", REF_VARIANTS, ids=_id)
def test_reference_headers_match_model_and_library(lib_run, ref_run, key):
    """The same source against the reference's include tree: its arenas equal the model's (each at
    its own run's addresses) and, the addresses' alignment being what the model takes from them, this
    library's."""
    assert _judge(ref_run, key, only_ref=True) > 0
    for c in C.CASES:
        if (c.group, c.op, c.p0, c.p1) == key and c.ref:
            msg = C.first_difference(c, lib_run[1][c.idx][1], ref_run[1][c.idx][1], lib_run[0])
            assert msg is None, "library (got) against reference (want): " + msg

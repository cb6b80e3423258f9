"""CPU: the arithmetic of the deflate's length-limited code build and run-length header
(deflate.hpp_amd/csrc/huff_fit.h: init_len, fit_classes, plan_run), which deflate_kernels.hip
compiles into the emission kernels and shares with this test.

tests/cpp/huff_fit_test.cpp is a stand-alone program (its own main, no HIP, no GPU) that this
test compiles itself with g++: once plain, once with AddressSanitizer + UBSan.  Both binaries are
run directly -- nothing is preloaded.  It checks fit_classes (complete code inside the limit on
fuzzed and on every small class-size vector; the slack fill always ends on an empty remainder),
init_len against long double, plan_run against RFC 1951 and the greedy encoding, and prints the
cost of the build above package-merge.

tests/huff_model.py, the sequential Python model the GPU test trusts, is pinned to that program's
--lengths / --plan output, and the level-1 families of tests/entropy_cases.py are checked, on the
model alone, to reach the branches they are there for."""
import os
import random
import shutil
import subprocess

import pytest

import entropy_cases as EC
import huff_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "huff_fit_test.cpp")


def _build(tmp_path, name, extra):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *extra, SRC, "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0:
        if extra and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
            pytest.skip("g++ without the sanitizer runtimes: " + r.stderr[-200:])
        raise AssertionError(r.stderr[-3000:])
    return exe


def _run(exe, args=(), stdin=None, env=None):
    r = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r


def _check_report(r):
    assert "[FAIL]" not in r.stderr and " 0 failed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    lines = r.stdout.splitlines()
    passes = [l for l in lines if "slack-fill passes, maximum" in l]
    assert passes and int(passes[0].split("maximum")[1].split()[0]) < 64, r.stdout[-3000:]
    for alpha in ("lit", "dist", "pre"):
        assert any(l.startswith("excess fuzz") and f" {alpha} " in l for l in lines), r.stdout[-3000:]
    assert any(l.startswith("excess level-1 ") and "worst" in l for l in lines), r.stdout[-3000:]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("huff_fit"), "huff_fit_test", [])


def test_huff_fit_plain(exe):
    r = _run(exe)
    print(r.stdout)
    _check_report(r)


def test_huff_fit_under_asan_ubsan(tmp_path):
    san = _build(tmp_path, "huff_fit_test_san",
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = _run(san, env=env)
    _check_report(r)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


# ---- the Python model against the program that runs the kernels' functions ------------------------
def _fuzz_hist(rng, nsym):
    used = rng.randint(0, nsym) if rng.random() < 0.9 else rng.randint(0, 2)
    f = [0] * nsym
    kind = rng.randrange(5)
    q, g = rng.choice((0.5, 0.7, 0.9, 0.97, 0.99)), 60000.0
    for i, s in enumerate(rng.sample(range(nsym), used)):
        if kind == 0:
            v = rng.randint(1, 3)
        elif kind == 1:
            v = int(2 ** (16 * rng.random()))
        elif kind == 2:
            v, g = int(g), g * q
        elif kind == 3:
            v = rng.randint(20000, 60000) if i == 0 else rng.randint(1, 4)
        else:
            v = rng.randint(1, 2000)
        f[s] = max(1, v)
    return f


def _family_hists():
    """The lit/len histograms of every named level-1 family at every segment size."""
    out = []
    for name, w in EC.FAMILIES.items():
        for n in EC.SEGS + (1, 777, 5000):
            h = EC.counts(w, n) + [1] + [0] * 29
            out.append(h)
    return out


def test_model_lengths_equal_the_shared_functions(exe):
    rng = random.Random(20240)
    jobs = []
    for alpha in (HM.LIT, HM.DIST, HM.PRE):
        jobs += [(alpha, _fuzz_hist(rng, alpha[1])) for _ in range(5000)]
    jobs += [(HM.LIT, h) for h in _family_hists()]
    text = "".join(f"{a[0]} {' '.join(map(str, f))}\n" for a, f in jobs)
    got = _run(exe, ["--lengths"], stdin=text).stdout.splitlines()
    assert len(got) == len(jobs)
    for (alpha, f), line in zip(jobs, got):
        assert HM.lengths(f, alpha) == [int(x) for x in line.split()], (alpha[0], f)


def test_model_plan_run_equals_the_shared_function(exe):
    jobs = [(v, r) for v in range(16) for r in range(1, 317)]
    got = _run(exe, ["--plan"], stdin="".join(f"{v} {r}\n" for v, r in jobs)).stdout.splitlines()
    assert len(got) == len(jobs)
    for (v, r), line in zip(jobs, got):
        n18, last18, n17, r17, nlit, n16, last16 = (int(x) for x in line.split())
        if v == 0:
            want = [(18, 138)] * (n18 - 1) + [(18, last18)] * min(n18, 1) + [(17, r17)] * n17 + [(0, 1)] * nlit
        else:
            want = [(v, 1)] + [(16, 6)] * (n16 - 1) + [(16, last16)] * min(n16, 1) + [(v, 1)] * (nlit - 1)
        assert HM.plan_run(v, r) == want, (v, r)


# ---- the families reach what they are there for (the model alone) -----------------------------------
def _model_block(name, n, final=False):
    return HM.block(EC.counts(EC.FAMILIES[name], n) + [0] * 30, [0] * 30, n, final)


def _runs(lens):
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        out.append((lens[i], j - i))
        i = j
    return out


@pytest.mark.parametrize("seg", EC.SEGS)
def test_families_reach_their_branches(seg):
    for m in (130, 200, 255):
        b = _model_block(f"near-uniform {m}", seg)
        assert b.lit.moved >= 30, (m, b.lit.moved)  # the repair lengthens dozens of symbols
        assert b.btype == 2
    assert _model_block("geometric 0.5", seg).lit.clamped >= 200
    assert _model_block("fibonacci 22", seg).lit.clamped >= 1
    for final in (False, True):
        assert _model_block("uniform 256", seg, final).btype == 0
        # 255 equally frequent values and the end-of-block are 256 codes of 8 bits: no code beats
        # the stored form (log2 255 = 7.994 bits a byte, the header costs more than the rest), so
        # the largest alphabets that come out dynamic are uniform 200 and near-uniform 255
        assert _model_block("uniform 255", seg, final).btype == 0
        assert _model_block("uniform 200", seg, final).btype == 2
        assert _model_block("near-uniform 255", seg, final).btype == 2
        assert _model_block("uniform 1", seg, final).btype == 2
    for name, (_, want) in EC.ZERO_RUNS.items():
        b = _model_block(name, seg)
        assert b.btype == 2, name
        zr = [r for v, r in _runs(b.litlens[:b.hdr.hlit]) if v == 0]
        for r in want:
            assert r in zr, (name, r, zr)
    b = _model_block("zero run 254", seg)
    assert b.litlens[255] == 0 and _runs(b.litlens[:257])[-2] == (0, 254)  # the run ends at symbol 255
    for name, (_, want) in EC.EQUAL_RUNS.items():
        b = _model_block(name, seg)
        assert b.btype == 2, name
        nz = [r for v, r in _runs(b.litlens[:b.hdr.hlit]) if v]
        for r in want:
            assert r in nz, (name, r, nz)
    # the header's symbols: every arm of plan_run occurs somewhere in the families
    seen = set()
    for name in EC.FAMILIES:
        seen |= {(s, rep) for s, rep in _model_block(name, seg).hdr.syms if s >= 16}
    for need in [(18, 138), (18, 116), (18, 11), (17, 3), (17, 10), (16, 3), (16, 6), (16, 4), (16, 5)]:
        assert need in seen, need


def test_sweep_reaches_every_block_type():
    import dmx
    bufs = EC.sweep_buffers(dmx.corpus("text", 1300))
    assert len(bufs) == 1800
    # stored needs byte values above 143 (see sweep_buffers): the 16-value alphabet shows all three
    # block types, the other two the fixed and the dynamic one
    want = {"two values": {1, 2}, "16 values geometric": {0, 1, 2}, "text": {1, 2}}
    for alpha in EC.SWEEP_ALPHABETS:
        types = {HM.block(HM.byte_hist(d), [0] * 30, len(d), True).btype for a, d in bufs if a == alpha}
        assert types == want[alpha], (alpha, types)

"""What avcer_conv_gemm's dtype means and which form and tile serves a shape (avcer_amd/csrc/gemm_forms.h), on the CPU: the header
includes nothing of HIP, so tests/gemm_forms_driver.cpp compiles with the host compiler alone."""
import csv
import itertools
import os
import shutil
import subprocess

import pytest

from avcer_amd import build
from test_gpu_kernels import A_KIND, O_KIND

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("f32", "bf16", "sp32")                     # KIND_*
STAGED, DIRECT, SKINNY = 0, 1, 2                    # FORM_*
COLUMNS = ("M", "N", "cin", "kh", "kw", "pad", "groups", "x2_cin", "tile_n", "tile_m", "slots", "a_kind", "o_kind", "x3", "copies", "short_in")


def shape(M, N, cin, kh=1, kw=1, pad=0, groups=0, x2_cin=0, tile_n=0, tile_m=0, slots=512, a_kind=2, o_kind=2, x3=1, copies=15, short_in=0):
    return (M, N, cin, kh, kw, pad, groups, x2_cin, tile_n, tile_m, slots, a_kind, o_kind, x3, copies, short_in)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """run(shapes) -> (table rows {dtype: fields}, other lines {name: ints}, per shape (dtype, tile, why not direct, why not skinny))"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gemm_forms") / "gemm_forms_driver")
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", build.CSRC, os.path.join(HERE, "gemm_forms_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(shapes=()):
        text = "".join(" ".join(str(int(v)) for v in s) + "\n" for s in shapes)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        table, vals, choices = {}, {}, []
        for line in out.stdout.splitlines():
            if line.startswith("choice "):
                head, no_direct, no_skinny = line[len("choice "):].split("|")
                choices.append(tuple(int(v) for v in head.split()) + (no_direct, no_skinny))
            else:
                f = line.split()
                if f[0] == "row":
                    names = ("a_kind", "o_kind", "w_copy", "form", "mode", None, "inverse", None, "in_bytes", "out_bytes", None, "bk", None, "a_split",
                             None, "ovec", None, "family")
                    table[int(f[1])] = {n: int(v) for n, v in zip(names, f[2:]) if n}
                else:
                    vals[f[0]] = [int(v) for v in f[1:]]
        assert len(choices) == len(shapes)
        return table, vals, choices

    return run


def test_table_is_the_tests_table(driver):
    """The header's row of every dtype reads / writes what the tests' own A_KIND / O_KIND say, gemm_dtype of a row's own fields is that
    row, and what the launcher derives from a row is what the storage kinds imply."""
    table, vals, _ = driver()
    assert sorted(table) == sorted(A_KIND) == sorted(O_KIND) == list(range(11))
    for dtype, row in table.items():
        assert KINDS[row["a_kind"]] == A_KIND[dtype] and KINDS[row["o_kind"]] == O_KIND[dtype], dtype
        assert row["inverse"] == dtype
        assert row["in_bytes"] == (2 if A_KIND[dtype] == "bf16" else 4) and row["out_bytes"] == (2 if O_KIND[dtype] == "bf16" else 4)
        assert row["bk"] * row["in_bytes"] == 128 and row["a_split"] == (A_KIND[dtype] == "sp32")
        assert row["ovec"] == {"f32": 4, "bf16": 8, "sp32": 32}[O_KIND[dtype]]
        assert row["form"] == (STAGED if dtype < 7 else DIRECT if dtype < 9 else SKINNY)
        assert row["family"] == {STAGED: 0, DIRECT: 1, SKINNY: 5}[row["form"]]  # AVCER_FAM_GEMM, _GEMM_WD, _SKINNY
        assert row["w_copy"] == (3 if dtype >= 7 else 2 if dtype >= 3 else 1 if dtype >= 1 else 0)
    assert vals["inverse_none"] == [-1, -1]
    assert vals["splits"] == [1, 0, 0, 0]


def test_chooser_never_picks_a_refused_form(driver):
    """Over a grid of shapes (both sides of every tile multiple and threshold, one and sixteen groups, with and without a second
    source and a short input, every hint, two slot counts): the form choose_gemm picks is one its own predicate takes."""
    ms = sorted({m + e for m in (1, 16, 32, 64, 112, 128, 512, 2048, 4096, 14336, 65536, 3097600) for e in (-1, 0, 1)} - {0})
    hints = ((0, 0), (64, 0), (128, 0), (256, 0), (0, 16), (0, 64), (0, 112), (0, 128))
    shapes = [shape(m, n, k - x2, groups=g, x2_cin=x2, tile_n=tn, tile_m=tm, slots=sl, o_kind=ok, short_in=sh)
              for m, n, k, (g, x2, sh), (tn, tm), sl, ok in itertools.product(ms, (64, 192, 256, 1024), (96, 128, 160, 1024), ((0, 0, 0), (16, 0, 0), (0, 64, 0), (0, 64, 1)), hints,
                                                                              (128, 512), (2, 0))]
    table, _, choices = driver(shapes)
    forms = set()
    for s, (dtype, tile, no_direct, no_skinny) in zip(shapes, choices):
        assert dtype >= 5, s
        form = table[dtype]["form"]
        forms.add(form)
        assert not (form == DIRECT and no_direct != "-") and not (form == SKINNY and no_skinny != "-"), (s, dtype, no_direct, no_skinny)
        assert tile in {STAGED: (64, 128), DIRECT: (112, 128), SKINNY: (16, 32, 64)}[form], (s, dtype, tile)
    assert forms == {STAGED, DIRECT, SKINNY}


def test_golden_choices(driver):
    """tests/golden/gemm_forms.csv: the dtype and tile (tile_m of the direct and the skinny form, width of the staged one) that the
    selection code chose before it moved into gemm_forms.h, for the contraction shapes of the networks at 1 .. 1024 frames or
    windows, both sides of every threshold and every hint."""
    with open(os.path.join(HERE, "golden", "gemm_forms.csv")) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) > 300
    _, _, choices = driver([tuple(int(r[c]) for c in COLUMNS) for r in rows])
    wrong = [(r["name"], (int(r["dtype"]), int(r["tile"])), c[:2]) for r, c in zip(rows, choices) if (int(r["dtype"]), int(r["tile"])) != c[:2]]
    assert not wrong, wrong[:10]
    assert {int(r["dtype"]) for r in rows} == set(range(-1, 11))


def test_refusals(driver):
    """One shape for each reason a predicate gives; (M 100000 or 100, N 512, K 512) itself is taken by the direct / the skinny form."""
    direct_shape, x2_gather, skinny_shape = "needs N % 256 == 0, an even number of K-steps, one group", "with a second source needs a pad-free gather", \
        "(skinny form) needs one source, cin % 32 == 0, n % 32 == 0, M <= 4096"
    cases = [(shape(100000, 512, 512), "-", None), (shape(100000, 384, 512), direct_shape, None), (shape(100000, 512, 480), direct_shape, None),
             (shape(100000, 512, 512, groups=2), direct_shape, None), (shape(100000, 512, 512, tile_n=64), direct_shape, None),
             (shape(100000, 512, 512, tile_n=128), direct_shape, None), (shape(100000, 512, 448, x2_cin=64), "-", None),
             (shape(100000, 512, 448, x2_cin=64, short_in=1), x2_gather, None),
             (shape(100, 512, 512), None, "-"), (shape(4096, 512, 512), None, "-"), (shape(4097, 512, 512), None, skinny_shape),
             (shape(100, 512, 448, x2_cin=64), None, skinny_shape), (shape(100, 512, 48), None, skinny_shape), (shape(100, 528, 512), None, skinny_shape)]
    _, _, choices = driver([c[0] for c in cases])
    for (s, no_direct, no_skinny), got in zip(cases, choices):
        assert no_direct is None or got[2] == no_direct, (s, got)
        assert no_skinny is None or got[3] == no_skinny, (s, got)
    assert choices[0][0] == 7 and choices[8][0] == 9

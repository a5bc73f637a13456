"""The choosers of csrc/acgpu_forms.h on the CPU: tests/tile_forms.cpp, a stand-alone host program, sweeps a grid of tables and
launches through choose_tile_form, choose_ww_form and choose_dfa_form.  For every input the kernel's name, its dynamic LDS and
(k_ac_tile) its ten template arguments must be what tests/tile_forms_expected.txt lists: that list was printed, for the same
sweep, by the dispatch code the choosers replaced -- the launch_* templates, switch blocks and macro ladders of acgpu_tile.hip,
acgpu_wholeword.hip and acgpu_kernels.hip, linked against stub launches that recorded the instantiation they were given.  `none`:
that code refused the input (hipErrorInvalidValue).  Every chosen form must be in the table of compiled forms, and the sweep
reaches every entry of the tables."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# table entries the sweep cannot reach, with the reason (at most 8): none -- every compiled form is chosen for some input
UNREACHED = {}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        pytest.skip("no ROCm clang++")
    exe = tmp_path_factory.mktemp("tile_forms") / "tile_forms"
    csrc = os.path.join(ROOT, "ahocorasick_amd", "csrc")
    subprocess.check_call([clang, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wno-c++20-extensions", "-Wno-unused-function", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", str(exe),
                           os.path.join(ROOT, "tests", "tile_forms.cpp")])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace").splitlines()
    assert p.returncode == 0 and out[-1] == "tile_forms: done" and "runtime error:" not in p.stdout.decode(errors="replace"), out[-20:]
    return out[:-1]


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(ROOT, "tests", "tile_forms_expected.txt")) as f:
        return f.read().splitlines()


def test_every_input_takes_the_kernel_the_old_dispatch_took(sweep, expected):
    got = [ln for ln in sweep if not ln.startswith("unreached ")]
    assert len(got) == len(expected) > 800
    wrong = [(g, e) for g, e in zip(got, expected) if g != e]
    assert not wrong, wrong[:5]
    assert not any(ln.startswith("NOT COMPILED") for ln in got)


def test_the_sweep_reaches_every_compiled_form(sweep, expected):
    unreached = [ln[len("unreached "):] for ln in sweep if ln.startswith("unreached ")]
    assert len(UNREACHED) <= 8 and sorted(unreached) == sorted(UNREACHED), unreached
    # ... and so did the old dispatch: 116 instantiations of k_ac_tile, 12 + 3 WholeWord names, 8 + 3 of the chunk scan
    results = [ln.split(" -> ")[1] for ln in expected if not ln.endswith("-> none")]
    tile = {r.split(", ")[-1] for r in results if r.startswith("k_ac_tile<")}
    assert len(tile) == 116 - len([u for u in UNREACHED if u.startswith("k_ac_tile")])
    names = {r.split(">")[0] + ">" if "<" in r else r for r in results}
    count = lambda prefix: len([n for n in names if n.startswith(prefix)])
    assert (count("k_ww_pp<"), count("k_ww_tile<"), count("k_ac_dfa<"), count("k_ac_scan_")) == (12, 3, 8, 3), sorted(names)


def test_the_names_of_the_large_second_level_are_cut_to_the_abi_field(expected):
    """BIG prints ten arguments, 68 to 70 characters: acgpu_profile::scan_kernel holds 63"""
    tile = [ln.split(" -> ")[1].rsplit(", ", 2) for ln in expected if " -> k_ac_tile<" in ln]  # name, LDS, arguments
    big = [name for name, _, args in tile if args.endswith(" 1")]  # (the tenth argument)
    assert big and all(len(n) == 63 and n.startswith("k_ac_tile<4, ") and not n.endswith(">") for n in big), big[:3]
    assert all(len(name) < 63 and name.endswith(">") for name, _, args in tile if args.endswith(" 0"))

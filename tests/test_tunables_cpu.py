"""acgpu_set_tunable against the list of knobs (ACGPU_TUNABLES, csrc/acgpu_internal.h): every name reaches a slot of its own, and
every slot starts at its default.  The knobs are process-global, so the calls are made in a fresh child process that loads the
library and nothing else; no device is needed."""
import json
import subprocess
import sys

from ahocorasick_amd import _native as N

# (name, default) of every knob, as struct Tunables listed them before the list existed.  filter_max_bytes: the default of a
# build without -DACGPU_FILTER_MAX_BYTES.
KNOBS = [
    ("chunk_units", 0),
    ("blocks_per_cu", 1),
    ("lds_table_bytes", 127 * 1024),
    ("force_sparse", 0),
    ("dense_budget_bytes", 1 << 30),
    ("force_kernel", 0),
    ("region_units", 0),
    ("rdense_budget_bytes", 256 << 20),
    ("tile_debug", 0),
    ("filter_max_bytes", 88000),
    ("no_short_keywords", 0),
    ("no_merged_ranges", 0),
    ("ww_block", 0),
    ("ww_ramp_pm", -1),
    ("ww_no_byte_pages", 0),
    ("ww_no_ph", 0),
    ("ww_ph_lambda", 0),
    ("ww_no_bloom", 0),
    ("ww_first_seed", 0),
    ("split_cand_div", 8),
    ("no_class_pages", 0),
    ("no_big_l2", 0),
    ("multi_min_share", 1 << 22),
    ("longest_form", 0),
    ("all_form", 0),
    ("no_state_form", 0),
    ("no_bits_trie", 0),
    ("reserve_cus", 0),
    ("tile_form", 0),
    ("cursor_first_piece", 1 << 20),
    ("cursor_max_piece", 1 << 26),
    ("cursor_reservoir_bytes", 256 << 20),
    ("states_chunk_log2", 0),
    ("replace_slab_units", 1 << 25),
    ("count_form", 0),
]

CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
L.acgpu_set_tunable.restype = ctypes.c_int64
L.acgpu_set_tunable.argtypes = [ctypes.c_char_p, ctypes.c_int64]
knobs = json.loads(sys.argv[2])
out = {"knobs": []}
# first every knob once with its default (what came back is what the slot held at the start), only then the changes: a name that
# reached another knob's slot would find that slot's value there, not its own default
first = [L.acgpu_set_tunable(name.encode(), dflt) for name, dflt in knobs]
for (name, dflt), at_start in zip(knobs, first):
    second = L.acgpu_set_tunable(name.encode(), dflt + 1)
    third = L.acgpu_set_tunable(name.encode(), dflt)
    out["knobs"].append([name, at_start, second, third])
# a value of its own into every knob, then all of them read back: two names that shared a slot would see each other's
out["distinct_set"] = [L.acgpu_set_tunable(name.encode(), 1000 + i) for i, (name, dflt) in enumerate(knobs)]
out["distinct_back"] = [L.acgpu_set_tunable(name.encode(), dflt) for name, dflt in knobs]
out["unknown"] = [L.acgpu_set_tunable(b"no_such_knob", 1), L.acgpu_set_tunable(b"", 1), L.acgpu_set_tunable(None, 1)]
a0 = L.acgpu_set_tunable(b"ablation_build", 0)
a1 = L.acgpu_set_tunable(b"ablation_build", 7)
a2 = L.acgpu_set_tunable(b"ablation_build", 0)
out["ablation"] = [a0, a1, a2]
print(json.dumps(out))
"""


def test_every_tunable_reaches_its_own_slot_and_starts_at_its_default():
    assert len(KNOBS) == len({name for name, _ in KNOBS}) == 35
    p = subprocess.run([sys.executable, "-c", CHILD, N.LIB_PATH, json.dumps(KNOBS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    got = json.loads(p.stdout.decode().strip().splitlines()[-1])
    assert [k[0] for k in got["knobs"]] == [name for name, _ in KNOBS]
    for (name, dflt), (_, at_start, second, third) in zip(KNOBS, got["knobs"]):
        assert at_start == dflt, (name, "starts at", at_start)        # set(name, default) returns the default
        assert second == dflt, (name, "second call saw", second)      # set(name, default + 1) returns the default as well
        assert third == dflt + 1, (name, "third call saw", third)     # set(name, default) after that returns default + 1
    assert got["distinct_set"] == [dflt for _, dflt in KNOBS]
    assert got["distinct_back"] == [1000 + i for i in range(len(KNOBS))]
    assert got["unknown"] == [-1, -1, -1]
    a0, a1, a2 = got["ablation"]
    assert a0 in (0, 1) and a1 == a0 and a2 == a0  # read only: an attempt to set it changes nothing

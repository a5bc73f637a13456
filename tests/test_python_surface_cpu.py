"""The public surface of ahocorasick_amd/strings.py (no GPU, no library): every public method and property of the binding classes
and of the ten matcher classes, inherited ones included, with its signature, against tests/golden/python_surface.json.  A method
that moves to a base class, or is written once for Set and Map, keeps its name, its parameter names and its defaults."""
import inspect
import json
import os

from ahocorasick_amd import strings as S

CLASSES = ["Automaton", "Comm", "Ticket", "Stream", "Cursor", "StringSet", "StringMap",
           "AhoCorasickSet", "AhoCorasickMap", "LongestMatchSet", "LongestMatchMap", "ShortestMatchSet", "ShortestMatchMap",
           "WholeWordMatchSet", "WholeWordMatchMap", "WholeWordLongestMatchSet", "WholeWordLongestMatchMap"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_surface.json")


def surface():
    """{"Class.name": signature | "property"} over the public names of each class and its constructor"""
    out = {}
    for cls_name in CLASSES:
        cls = getattr(S, cls_name)
        out[cls_name + ".__init__"] = str(inspect.signature(cls.__init__))
        for name in dir(cls):
            if name.startswith("_"):
                continue
            member = inspect.getattr_static(cls, name)
            if isinstance(member, property):
                out["%s.%s" % (cls_name, name)] = "property"
            elif callable(member):
                out["%s.%s" % (cls_name, name)] = str(inspect.signature(getattr(cls, name)))
    return out


def test_public_methods_and_signatures_are_those_of_the_golden_file():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = surface()
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert {k: v for k, v in got.items() if want[k] != v} == {}
    assert len(want) > 129  # (129 were counted over a subset of these classes)

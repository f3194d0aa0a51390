"""What the CPU tests ask of the reference's source, answered from data (tests/golden/reference_facts.json) so that they run without a
reference checkout.  A query names a file relative to the reference's root (or ALL_RS: every .rs file under src/ and benches/src/) and a
substring or a regex; the answer is whether the reference has it.

To re-record the answers from a checkout of the reference:
    AVN_REFERENCE_DIR=<checkout> python -m pytest tests/test_rust_layer_cpu.py tests/test_reference_fixtures.py -m "not gpu"
In that mode every query is answered from the checkout and the JSON is rewritten, at the end of the run, with the answers the run asked for."""
import atexit
import functools
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_facts.json")
ALL_RS = "src/**/*.rs + benches/src/**/*.rs"
_LIVE = os.environ.get("AVN_REFERENCE_DIR")
_facts = None
_recorded = {}


@functools.lru_cache(maxsize=None)
def _text(rel):
    if rel == ALL_RS:
        out = []
        for root in (os.path.join(_LIVE, "src"), os.path.join(_LIVE, "benches", "src")):
            for d, _, files in os.walk(root):
                for f in files:
                    if f.endswith(".rs"):
                        out.append(open(os.path.join(d, f), errors="replace").read())
        return "\n".join(out)
    return open(os.path.join(_LIVE, rel)).read()


def _answer(rel, kind, query):
    if _LIVE:
        if kind == "exists":
            got = os.path.exists(os.path.join(_LIVE, rel))
        elif kind == "contains":
            got = query in _text(rel)
        else:
            got = re.search(query, _text(rel)) is not None
        _recorded.setdefault(rel, {}).setdefault(kind, {})[query] = got
        return got
    global _facts
    if _facts is None:
        _facts = json.load(open(GOLDEN))["files"]
    try:
        return _facts[rel][kind][query]
    except KeyError:
        raise AssertionError(f"{GOLDEN} holds no answer for {kind} {query!r} in {rel}: re-record it (see tests/reference_facts.py)") from None


def exists(rel):
    return _answer(rel, "exists", "")


def contains(rel, needle):
    return _answer(rel, "contains", needle)


def search(rel, pattern):
    return _answer(rel, "search", pattern)


@atexit.register
def _write():
    if not (_LIVE and _recorded):
        return
    data = {"about": "answers of the reference's source to the queries of tests/reference_facts.py (file relative to the reference's root; "
                     "'exists', or a substring / regex -> found)", "files": {}}
    if os.path.exists(GOLDEN):
        data["files"] = json.load(open(GOLDEN))["files"]
    for rel, kinds in _recorded.items():
        for kind, answers in kinds.items():
            data["files"].setdefault(rel, {}).setdefault(kind, {}).update(answers)
    with open(GOLDEN, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")

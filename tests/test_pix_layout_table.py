"""The layout table of vittracker_amd/pixfmt.py against the behaviour recorded before it existed (tests/golden/ref_pix_layouts.json, written
by tests/golden/make_golden_pix_layouts.py from ImageTable.check with its twelve sets of layout codes and the eight plane validators of
the Image constructors), and against the codes include/vittrack.h defines.  CPU only."""
import importlib.util
import json
import os
import re

import pytest

from conftest import GOLDEN_DIR, REPO


@pytest.fixture(scope="module")
def sweep():
    """(recorded, replayed): the committed file and what the recording script gets from the code as it is now."""
    from vittracker_amd import native
    spec = importlib.util.spec_from_file_location("make_golden_pix_layouts", os.path.join(GOLDEN_DIR, "make_golden_pix_layouts.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    with open(os.path.join(GOLDEN_DIR, "ref_pix_layouts.json")) as f:
        recorded = json.load(f)
    return recorded, json.loads(json.dumps(mg.record(native)))      # through JSON: tuples as lists, integer keys as strings


def test_check_gives_the_recorded_outcome_for_every_code_and_case(sweep):
    recorded, now = sweep
    assert now["fragments"] == recorded["fragments"] and now["check_cases"] == recorded["check_cases"]
    per_code = lambda d: {c: s.split(";") for s, codes in d["check"].items() for c in codes}      # noqa: E731
    was, is_ = per_code(recorded), per_code(now)
    assert sorted(was) == sorted(is_) == list(range(256))
    labels = recorded["check_cases"]
    for code in range(256):
        assert len(was[code]) == len(is_[code]) == len(labels)
        for label, a, b in zip(labels, was[code], is_[code]):
            assert a == b, f"layout code {code}, case {label!r}: recorded {a}, now {b}"


def test_constructors_give_the_recorded_images(sweep):
    recorded, now = sweep
    assert list(now["constructors"]) == list(recorded["constructors"])
    for key, was in recorded["constructors"].items():
        assert now["constructors"][key] == was, f"{key}: recorded {was}, now {now['constructors'][key]}"


def test_table_has_the_codes_of_the_header_and_the_names(sweep):
    from vittracker_amd import native, pixfmt
    with open(os.path.join(REPO, "include", "vittrack.h")) as f:
        src = f.read()
    # the layouts are the enum's `VT_PIX_X = n` and the `#define VT_PIX_X n` with a decimal n (the colour tags are written in hex)
    header = {int(n): name.lower() for name, n in re.findall(r"\bVT_PIX_(\w+) = (\d+)\b", src)}
    header.update({int(n): name.lower() for name, n in re.findall(r"^#define VT_PIX_(\w+) (\d+)\s*$", src, re.M)})
    assert len(header) == 34, sorted(header.items())
    assert {c: L.name for c, L in pixfmt.LAYOUTS.items()} == header
    assert all(L.code == c for c, L in pixfmt.LAYOUTS.items())
    assert native.PIX_LAYOUT_NAMES == {c: L.name for c, L in pixfmt.LAYOUTS.items()} == {int(c): n for c, n in sweep[0]["names"].items()}
    assert all(getattr(native, "PIX_" + L.name.upper()) == c for c, L in pixfmt.LAYOUTS.items())


def test_pixfmt_imports_without_torch():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", "import sys, vittracker_amd.pixfmt; assert 'torch' not in sys.modules, 'pixfmt imported torch'"],
                       cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

"""Every validation answer of the operators' C entry points, byte for byte: return code and f3dgs_last_error() text.

tests/golden/make_entry_validation.py holds the call list (and how entry_validation.json was recorded: from the library of the
commit before the entry points moved out of api.hip into their units).  No call of the list passes its validation, so nothing
here reaches a HIP call: the test needs no GPU."""
import ctypes
import importlib.util
import json
import os

from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_entry_validation", os.path.join(GOLDEN, "make_entry_validation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_points_answer_as_recorded():
    from test_abi_and_surface import _ensure_built
    import torch  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    rec = _recorder()
    want = json.load(open(os.path.join(GOLDEN, "entry_validation.json")))
    got = rec.replay(ctypes.CDLL(_ensure_built()))
    assert [(r["fn"], r["label"]) for r in got] == [(r["fn"], r["label"]) for r in want], "the call list and the recording differ"
    wrong = [f"{w['fn']} [{w['label']}]: recorded {w['rc']} {w['error']!r}, got {g['rc']} {g['error']!r}"
             for w, g in zip(want, got) if (w["rc"], w["error"]) != (g["rc"], g["error"])]
    assert not wrong, "\n".join(wrong)


def test_the_list_covers_every_moved_entry_point_and_never_passes_validation():
    """Each of the 31 entry points that live in their operator's unit is called; every call that returns an int code either is
    refused (a message) or takes an early F3DGS_OK return, which its label says ("...: ok")."""
    rec = _recorder()
    want = json.load(open(os.path.join(GOLDEN, "entry_validation.json")))
    stay = {"f3dgs_contributions", "f3dgs_label_votes", "f3dgs_backward"}
    moved = set(rec.SIGNATURES) - stay
    assert len(moved) == 31 and moved <= {r["fn"] for r in want}
    assert stay <= {r["fn"] for r in want}
    for r in want:
        if rec.SIGNATURES[r["fn"]][0] is not rec.I:
            assert r["error"] is None
        elif r["label"].endswith(": ok"):
            assert r["rc"] == 0 and r["error"] is None, r
        else:
            assert r["rc"] < 0 and r["error"], r

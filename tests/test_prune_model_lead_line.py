"""The CPU model of bound pruning (profiles/prune_model.py) with the lead line: whichever way the leading strand's maximum is found -- its
line first, the other lanes certified, counted in full or counted again -- the read's maximum is the true one, for every read kind, and
reads without a match stay out of the part."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location(
    "prune_model", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prune_model.py"))
model = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(model)

KINDS = {"neg": (None, 0.0), "pos_fwd": (0, 0.075), "pos_rev": (1, 0.075), "near_fwd": (0, 0.16), "near_rev": (1, 0.16)}


def test_lead_line_keeps_the_maximum():
    rng = np.random.default_rng(7)
    taken = 0
    for name, kind in KINDS.items():
        for _ in range(3):
            r = model.read_lines(rng, kind)  # (asserts the maximum of every state against the counts itself)
            assert r["max_1234"] == r["true_max"], (name, r)
            assert r["line_held"] <= r["line_cert"] <= r["line_tried"], (name, r)
            if name == "neg":
                assert r["line_tried"] == 0 and r["1234"] == r["123"], r
            taken += r["line_tried"]
    assert taken >= 6  # the positives take it

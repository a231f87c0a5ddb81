"""What the audio-regression planners answer (no GPU, no launch):
ainp.janssen.plan_segments, ainp.janssen.plan_windows and
ainp.spain.plan_spain_windows on a fixed list of masks.

    python tests/golden/gen_window_plans.py     # writes window_plans.json

The fixture was written by the package as it stood before the two window
planners got one row loop and one table assembly (ainp/gaps.py);
tests/test_cpu_janssen_windowed.py asserts that the same masks still give the
same tables -- values, dtypes and shapes -- or the same ValueError text.

The cases: a support that starts before the signal (origin negative) and one
that overhangs its end; windows that lie inside the gap and get no row; two
signals with three gaps and two shapes; no gap at all; a run above 2048 in one
window (two window lengths) against a gap above 2048 for SPAIN; a second gap in
a window; SPAIN windows that wrap round the circular support; the bad (w, a)
pairs; segments clipped at both ends of their signals.  No mask was found that
reaches "falls into two runs of one window": with a | w the samples a window
leaves out, L - w of them, outnumber any gap the support was cut for.
"""
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "ml-audio-inpainting_amd")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "window_plans.json")


def mk(n, *gaps):
    """An all-observed mask of n samples with the [start, end) runs missing."""
    m = np.ones(n, bool)
    for a, b in gaps:
        m[a:b] = False
    return m


TWO = [mk(2000, (900, 980)), mk(1500, (300, 310), (1000, 1100))]
LONG = [mk(40000, (20000, 22100))]

# name -> (planner, masks, keyword arguments)
CASES = {
    "windows_origin_negative_3shapes": ("plan_windows", [mk(2000, (40, 120))],
                                        dict(p=32, w=256, a=64, wtypes=("hann", "rect", "tukey"))),
    "windows_overhang": ("plan_windows", [mk(2000, (1900, 1980))], dict(p=32, w=256, a=64)),
    "windows_all_missing_windows": ("plan_windows", [mk(800, (350, 440))], dict(p=8, w=64, a=16)),
    "windows_two_signals_two_shapes": ("plan_windows", TWO,
                                       dict(p=32, w=256, a=64, wtypes=("rect", "hann"))),
    "windows_no_gap": ("plan_windows", [mk(700)], dict(p=8, w=64, a=16)),
    "windows_run_2100": ("plan_windows", LONG, dict(w=4096, a=1024)),
    "windows_run_2074": ("plan_windows", LONG, dict(w=8192, a=2048)),
    "windows_second_gap": ("plan_windows", [mk(2000, (900, 980), (1100, 1110))],
                           dict(p=32, w=256, a=64)),
    "spain_tail": ("plan_spain_windows", [mk(2000, (1960, 2000))], dict(w=256, a=64)),
    "spain_head_wraps": ("plan_spain_windows", [mk(2000, (0, 40))], dict(w=256, a=64)),
    "spain_all_missing_windows": ("plan_spain_windows", [mk(800, (350, 440))], dict(w=64, a=16)),
    "spain_two_signals": ("plan_spain_windows", TWO, dict(w=256, a=64)),
    "spain_gap_2100": ("plan_spain_windows", LONG, dict(w=4096, a=1024)),
    "spain_second_gap": ("plan_spain_windows", [mk(2000, (900, 980), (1180, 1190))],
                         dict(w=256, a=64)),
    "segments_clipped": ("plan_segments", [mk(1000, (20, 50)), mk(1000, (950, 990))],
                         dict(w=100, p=16)),
}
for _w, _a in ((200, 50), (8192, 2048), (4, 2), (256, 60), (256, 256)):
    CASES[f"spain_bad_w{_w}_a{_a}"] = ("plan_spain_windows", [mk(2000, (900, 980))],
                                       dict(w=_w, a=_a))


def _plain(v):
    """A field as plain JSON types; arrays keep their dtype and shape."""
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype), "shape": list(v.shape), "values": v.tolist()}
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, (np.integer, np.floating)):
        return {"dtype": str(v.dtype), "shape": [], "values": v.item()}
    return v


def run_case(name):
    """{field: value} of the planner's result, or {"error": the ValueError text}."""
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ainp import janssen, spain
    fn, masks, kw = CASES[name]
    planner = getattr(spain if fn == "plan_spain_windows" else janssen, fn)
    try:
        plan = planner([m.copy() for m in masks], **kw)
    except ValueError as e:
        return {"error": str(e)}
    doc = {f.name: _plain(getattr(plan, f.name)) for f in dataclasses.fields(plan)}
    doc["len"] = len(plan)
    return doc


def main():
    doc = {name: run_case(name) for name in CASES}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    for name, d in doc.items():
        print(name, d["error"] if "error" in d else f"{d['len']} rows")
    print(OUT, len(doc), "cases")


if __name__ == "__main__":
    main()

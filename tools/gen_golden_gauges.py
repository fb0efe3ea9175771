#!/usr/bin/env python3
"""Golden data of the frame gauges, from the reference's OWN methods: Processor._autocrop_borders,
_is_real_letterbox_crop and _faceless_validate are taken out of the reference's person_capture/gui_app.py
by AST (the module itself does not import: Qt and cv2 are absent), detect_black_borders and _clamp out of
its utils.py, and run with a stub `self` (cfg, _status, _lock_last_bbox, _prev_gray) on the cases of
tests/frame_gauge_cases.py. The four cv2 calls they make get a NumPy stand-in, which is the stated
unpinned part: cvtColor(BGR2GRAY) is the oracle's gray_u8, absdiff / threshold /
countNonZero plain NumPy.

Writes data only, tests/golden/frame_gauges.npz:
  border_roi [cases][4], border_accepted [cases], border_real [cases] (_is_real_letterbox_crop of the
  clamped ROI), border_status [cases] (status messages emitted)
  motion_ok [cases], motion_reason [cases] (index into frame_gauge_cases.REASONS), motion_count [cases]
  (countNonZero's value, -1 where the reference never got there)
  clip_roi [frames][4], clip_accepted [frames], clip_ok / clip_reason / clip_count [frames][boxes]
Before writing, every strip statistic the reference computed (its own np.percentile and np.std values)
is asserted to lie further than 1e-3 from its threshold, and the largest relative difference between its
f32 np.std and this package's std_from_hist is printed. No reference source or bytecode is written anywhere.

Run: python tools/gen_golden_gauges.py <root of the reference snapshot>
"""
from __future__ import annotations

import ast
import math
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import frame_gauge_cases as fc  # noqa: E402

METHODS = ("_autocrop_borders", "_is_real_letterbox_crop", "_faceless_validate")
UTILS = ("_clamp", "detect_black_borders")


class Cv2StandIn:
    """The four cv2 calls of the lifted code."""
    COLOR_BGR2GRAY = 6
    THRESH_BINARY = 0

    def __init__(self):
        self.last_count = -1

    @staticmethod
    def cvtColor(img, code):
        from oracle.cv_ops import gray_u8
        assert code == Cv2StandIn.COLOR_BGR2GRAY
        return gray_u8(img)

    @staticmethod
    def absdiff(a, b):
        return np.abs(a.astype(np.int16) - b.astype(np.int16)).astype(np.uint8)

    @staticmethod
    def threshold(src, thresh, maxval, kind):
        assert kind == Cv2StandIn.THRESH_BINARY
        return float(thresh), np.where(src > thresh, maxval, 0).astype(np.uint8)

    def countNonZero(self, m):
        self.last_count = int(np.count_nonzero(m))
        return self.last_count


class NpRecorder:
    """numpy, with the strip statistics the reference computes written down as it computes them."""

    def __init__(self):
        self.stats = []   # (kind, value, number of samples, this package's value)

    def __getattr__(self, name):
        return getattr(np, name)

    def percentile(self, a, q, *args, **kw):
        v = np.percentile(a, q, *args, **kw)
        self.stats.append((f"p{int(q)}", float(v), a))
        return v

    def std(self, a, *args, **kw):
        v = np.std(a, *args, **kw)
        self.stats.append(("std", float(v), a))
        return v


def lift(path: str, names, ns: dict, in_class: bool) -> dict:
    src = open(path, encoding="utf-8").read()
    body = []
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name in names and node.name not in [b.name for b in body]:
            body.append(node)
    if sorted(b.name for b in body) != sorted(names):
        raise RuntimeError(f"{path} does not define " + ", ".join(names))
    for b in body:
        b.decorator_list = []
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, f"<{os.path.basename(path)} subset>", "exec"), ns)
    return {k: ns[k] for k in names}


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from typing import Tuple
    from person_capture_amd import frame_gauges as fg
    ref = sys.argv[1]
    cv2 = Cv2StandIn()
    rec = NpRecorder()
    uns = {"np": np, "cv2": cv2}
    U = lift(os.path.join(ref, "person_capture", "utils.py"), UTILS, uns, False)
    utils_mod = types.ModuleType("utils")
    utils_mod.detect_black_borders = U["detect_black_borders"]
    sys.modules["utils"] = utils_mod   # the lifted _autocrop_borders falls back to `from utils import ...`
    ns = {"np": rec, "cv2": cv2, "math": math, "Tuple": Tuple, "__name__": "lifted"}
    M = lift(os.path.join(ref, "person_capture", "gui_app.py"), METHODS, ns, True)

    class Stub:
        def __init__(self, cfg):
            self.cfg = cfg
            self.messages = []
            self._lock_last_bbox = None
            self._prev_gray = None

        def _status(self, msg, **kw):
            self.messages.append(msg)
    for k, f in M.items():
        setattr(Stub, k, f)

    border_cfg = types.SimpleNamespace(border_scan_frac=fc.SCAN_FRAC)

    def autocrop(frame):
        s = Stub(border_cfg)
        out, (ox, oy) = s._autocrop_borders(frame, fc.THR)
        h, w = out.shape[:2]
        roi = (ox, oy, ox + w, oy + h)
        accepted = out.shape != frame.shape
        # the ROI the reference validates, rebuilt as it builds it, for _is_real_letterbox_crop alone
        H, W = frame.shape[:2]
        max_scan = int(round(min(H, W) * fc.SCAN_FRAC))
        x1, y1, x2, y2 = U["detect_black_borders"](frame, thr=fc.THR, max_scan=max_scan)
        x1 = max(0, min(W - 1, int(x1))); y1 = max(0, min(H - 1, int(y1)))
        x2 = max(x1 + 1, min(W, int(x2))); y2 = max(y1 + 1, min(H, int(y2)))
        real = Stub(border_cfg)._is_real_letterbox_crop(frame, (x1, y1, x2, y2), fc.THR)
        return roi, accepted, real, len(s.messages)

    out = {}
    rois, acc, real, nmsg = [], [], [], []
    for name in fc.BORDER_NAMES:
        r, a, rl, m = autocrop(fc.border_frame(name))
        print(f"{name:22s} roi {r} accepted {a} real {rl} status messages {m}")
        rois.append(r); acc.append(a); real.append(rl); nmsg.append(m)
    out.update(border_roi=np.array(rois, np.int32), border_accepted=np.array(acc, bool),
               border_real=np.array(real, bool), border_status=np.array(nmsg, np.int32))

    def validate(stub, box, frame, lock):
        from oracle.cv_ops import gray_u8
        stub._lock_last_bbox = lock
        cv2.last_count = -1
        ok, reason = stub._faceless_validate(box, frame.shape, gray_u8(frame))
        return bool(ok), fc.REASONS.index(reason), cv2.last_count

    from oracle.cv_ops import gray_u8
    prev, cur = fc.motion_pair()
    res = []
    for box, cfg, lock in fc.MOTION_CASES:
        s = Stub(fc.CFGS[cfg])
        s._prev_gray = gray_u8(prev)
        res.append(validate(s, box, cur, lock))
        print(f"motion {box} {cfg} lock {lock}: {res[-1][0]} {fc.REASONS[res[-1][1]]} count {res[-1][2]}")
    out.update(motion_ok=np.array([r[0] for r in res], bool), motion_reason=np.array([r[1] for r in res], np.int32),
               motion_count=np.array([r[2] for r in res], np.int64))

    s = Stub(fc.CFG_OPEN)
    c_roi, c_acc, c_ok, c_reason, c_count = [], [], [], [], []
    for t in range(fc.CLIP_LEN):
        frame = fc.clip_frame(t)
        r, a, _, _ = autocrop(frame)
        per = [validate(s, b, frame, None) for b in fc.CLIP_BOXES]
        s._prev_gray = gray_u8(frame).copy()   # gui_app.py:8000
        c_roi.append(r); c_acc.append(a)
        c_ok.append([p[0] for p in per]); c_reason.append([p[1] for p in per]); c_count.append([p[2] for p in per])
        print(f"clip frame {t}: roi {r} accepted {a} boxes {per}")
    out.update(clip_roi=np.array(c_roi, np.int32), clip_accepted=np.array(c_acc, bool), clip_ok=np.array(c_ok, bool),
               clip_reason=np.array(c_reason, np.int32), clip_count=np.array(c_count, np.int64))

    # the reference's own strip statistics against their thresholds, and against this package's values
    max_luma = max(float(fc.THR) + 8.0, 18.0)
    limit = {"p95": max_luma, "p99": max_luma + 4.0, "std": fg.MAX_STD}
    worst_std = 0.0
    for kind, v, a in rec.stats:
        assert abs(v - limit[kind]) > 1e-3, (kind, v)
        hist = np.bincount(a.astype(np.uint8), minlength=256)
        if kind == "std":
            mine = fg.std_from_hist(hist)
            if mine > 0:
                worst_std = max(worst_std, abs(v - mine) / mine)
            else:
                assert v == 0.0
        else:
            assert fg.percentile_from_hist(hist, float(kind[1:])) == v, (kind, v)
    print(f"{len(rec.stats)} strip statistics, none within 1e-3 of its threshold; "
          f"largest relative |np.std f32 - std_from_hist| {worst_std:.3e}")
    out["std_rel_diff_max"] = np.array(worst_std)

    os.makedirs(os.path.dirname(fc.GOLDEN), exist_ok=True)
    np.savez_compressed(fc.GOLDEN, **out)
    print("->", fc.GOLDEN, os.path.getsize(fc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

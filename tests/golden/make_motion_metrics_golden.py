#!/usr/bin/env python3
"""tests/golden/motion_metrics.npz: known answers for the motion metrics, produced by EXECUTING the reference's own code.

`L1div` and `alignment.load_pose / calculate_align / GAHR / motion_frames2time` are lifted out of utils/metric.py, and `recover_root_rot_pos /
recover_from_ric` with `qinv / qrot` out of utils/plot_script.py and utils/quaternion.py, with `ast` at run time and compiled as they stand (the
modules' own imports - librosa, matplotlib - are never executed).  Nothing of them is stored: seeds, inputs and the reference's outputs only.
    python tests/golden/make_motion_metrics_golden.py

`smplx` is not installed, so the joints the metrics are run on come from tests/motion_metrics_ref.fk_oracle (fp64), rounded to float32 as the
reference's would arrive.  The take is a smooth random trajectory (band-limited noise on the rotations), its seed searched on the CPU until
  (a) every strict comparison the reference makes - a slice value against each of its `order` neighbours a side, every speed against the
      threshold - has a relative margin of at least MARGIN = 1e-4: fp32 device speeds of the same joints cannot flip a beat;
  (a') every OUTCOME is safe by ROBUST = 5e-3: a slice index is a beat with all its comparisons true by that margin, or is none with one of
      them false by that margin (a neighbour clipped onto the element itself compares equal in any precision).  This is what lets the
      end-to-end test start from the device's own fp32 joints: their error moves a speed by a few 1e-5 of itself;
  (b) some minimum is kept by the verbatim rule vel[j] > threshold and dropped by the "corrected" vel[j + t_start] > threshold, or the reverse;
  (c) some upper-body joint has no beats;
  (d) some upper-body joint has beats.
`build()` asserts all four for the seed it settles on.

Contents: take.{seed,n,t_start,t_end,order,sigma,fps}, take.rest (55, 3), take.aa (n, 55, 3), take.transl (n, 3), take.joints (n, 165), take.mmae (55,),
take.onsets; take.vel (n, 55) and take.vel_slice (n_slice, 55): what the reference handed to argrelextrema for the whole take and for the slice;
take.beats / take.beats_t0 (uint8 masks of load_pose's lists for the slice and for t_start = 0), take.beats_corrected (the other rule, from
the restatement), take.bc, take.per_joint, take.l1_sum / take.l1_avg (L1div on a float32 copy), take2.* (n = 2); ric.<case> (reference torch fp32).
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO  # noqa: E402

sys.path.insert(0, REPO)
from tests import motion_metrics_ref as mr  # noqa: E402

MARGIN, ROBUST = 1e-4, 5e-3
N, T_START, T_END, ORDER, SIGMA, FPS = 80, 16, 64, 7, 0.3, 30
QUIET_JOINT = 3            # an upper-body joint whose mmae is set so high that it never crosses the threshold: (c)


def lift(path, names, ns):
    tree = ast.parse(open(path).read(), filename=path)
    keep = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(keep) == len(names), (path, names)
    for n in keep:
        if isinstance(n, ast.ClassDef) and n.name == "alignment":
            n.body = [f for f in n.body if isinstance(f, ast.FunctionDef) and f.name in ("__init__", "load_pose", "calculate_align", "GAHR", "motion_frames2time")]
            assert len(n.body) == 5
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


def reference_metric():
    import math
    from scipy.signal import argrelextrema
    seen = []

    def recording(data, comparator, order=1, **kw):
        seen.append(np.array(data))
        return argrelextrema(data, comparator, order=order, **kw)
    ns = lift(os.path.join(REF, "utils", "metric.py"), ("L1div", "alignment"), {"np": np, "math": math, "argrelextrema": recording})
    return ns["L1div"], ns["alignment"], seen


def reference_ric():
    import torch
    ns = lift(os.path.join(REF, "utils", "quaternion.py"), ("qinv", "qrot"), {"torch": torch, "np": np})
    return lift(os.path.join(REF, "utils", "plot_script.py"), ("recover_root_rot_pos", "recover_from_ric"), ns)["recover_from_ric"]


def lists_to_mask(beats, n_slice):
    m = np.zeros((n_slice, len(beats)), dtype=np.uint8)
    for i, b in enumerate(beats):
        if len(b):
            m[np.asarray(b, dtype=np.int64), i] = 1
    return m


def take(seed):
    """Inputs of one candidate take."""
    rest = mr.synth_rest(0)
    aa = mr.smooth_rotations(seed, N)
    r = np.random.RandomState(seed + 500)                           # a slow sway of the root, so that joint 0 moves too
    transl = (0.1 * np.sin(2 * np.pi * r.uniform(0.2, 1.0, (1, 3)) * np.arange(N)[:, None] / FPS + r.uniform(0, 2 * np.pi, (1, 3)))).astype(np.float32)
    joints = mr.fk_oracle(mr.smplx_parents(), rest, aa, transl).astype(np.float32).reshape(N, 165)
    mmae = mr.speeds_ref(joints, FPS).mean(0) * 2.2                 # speeds / mmae scatter around 0.45: the 0.3 threshold is crossed both ways
    mmae[QUIET_JOINT] *= 40.0
    onsets = np.sort(np.random.RandomState(seed + 1000).uniform(0.0, (T_END - T_START) / FPS, 11))
    return rest, aa, transl, joints, mmae, onsets


def margins_ok(vel):
    """(a) on the reference's float64 speeds."""
    if (np.abs(vel - 0.3) < MARGIN * 0.3).any():
        return False
    s = vel[T_START:T_END]
    idx = np.arange(len(s))
    for k in range(1, ORDER + 1):
        for nb in (np.clip(idx + k, 0, len(s) - 1), np.clip(idx - k, 0, len(s) - 1)):
            real = nb != idx                                           # (a clipped neighbour that IS the element compares equal whatever the precision)
            a, b = s[real], s[nb[real]]
            if (np.abs(a - b) < MARGIN * np.maximum(np.abs(a), np.abs(b))).any():
                return False
    return True


def outcomes_robust(vel):
    """(a') on the reference's float64 speeds."""
    s = vel[T_START:T_END]
    m, idx = len(s), np.arange(len(s))
    sure_beat = vel[:m] > 0.3 * (1 + ROBUST)
    sure_none = vel[:m] < 0.3 * (1 - ROBUST)
    for k in range(1, ORDER + 1):
        for nb in (np.clip(idx + k, 0, m - 1), np.clip(idx - k, 0, m - 1)):
            d = (s[nb] - s) / np.maximum(np.abs(s[nb]), np.abs(s))
            self_cmp = (nb == idx)[:, None]
            sure_beat &= (d >= ROBUST) & ~self_cmp
            sure_none |= (d <= -ROBUST) | self_cmp
    return bool((sure_beat | sure_none).all())


def build():
    import torch
    L1div, alignment, seen = reference_metric()
    out = {}
    for seed in range(4000):
        rest, aa, transl, joints, mmae, onsets = take(seed)
        vel = mr.speeds_ref(joints, FPS, mmae, dtype=np.float32).astype(np.float64)      # a quick look before the reference is run
        if not (margins_ok(vel) and outcomes_robust(vel)):
            continue
        ver, cor = mr.beats_ref(vel, T_START, T_END, ORDER), mr.beats_ref(vel, T_START, T_END, ORDER, corrected=True)
        ub = mr.UPPER_BODY
        if (ver != cor).any() and any(ver[:, i].sum() == 0 for i in ub) and any(ver[:, i].sum() for i in ub):
            break
    else:
        raise SystemExit("no seed satisfies (a)-(d)")
    al = alignment(SIGMA, ORDER, mmae, upper_body=list(mr.UPPER_BODY))
    del seen[:]
    beats_t0 = al.load_pose(joints.copy(), 0, N, FPS, True)
    vel_ref = np.stack(seen, 1)                                        # the whole take, as argrelextrema saw it: (n, 55)
    del seen[:]
    beats = al.load_pose(joints.copy(), T_START, T_END, FPS, True)
    vel_slice = np.stack(seen, 1)
    assert (vel_slice == vel_ref[T_START:T_END]).all()
    mask, mask_t0 = lists_to_mask(beats, T_END - T_START), lists_to_mask(beats_t0, N)
    cor = mr.beats_ref(vel_ref, T_START, T_END, ORDER, corrected=True)
    assert margins_ok(vel_ref), "(a)"
    assert outcomes_robust(vel_ref), "(a')"
    assert (mask != cor).any(), "(b)"
    assert any(mask[:, i].sum() == 0 for i in mr.UPPER_BODY), "(c)"
    assert any(mask[:, i].sum() for i in mr.UPPER_BODY), "(d)"
    bc = al.calculate_align(onsets, beats, FPS)
    per_joint = [alignment.GAHR(alignment.motion_frames2time(b, 0, FPS), onsets, SIGMA) for i, b in enumerate(beats) if i in mr.UPPER_BODY]
    l1 = L1div()
    l1.run(joints.copy())
    out.update({"take.seed": np.int64(seed), "take.n": np.int64(N), "take.t_start": np.int64(T_START), "take.t_end": np.int64(T_END),
                "take.order": np.int64(ORDER), "take.sigma": np.float64(SIGMA), "take.fps": np.int64(FPS), "take.margin": np.float64(MARGIN), "take.robust": np.float64(ROBUST),
                "take.rest": rest, "take.aa": aa, "take.transl": transl, "take.joints": joints, "take.mmae": mmae, "take.onsets": onsets,
                "take.vel": vel_ref, "take.vel_slice": vel_slice, "take.beats": mask, "take.beats_t0": mask_t0, "take.beats_corrected": cor,
                "take.bc": np.float64(bc), "take.per_joint": np.asarray(per_joint, dtype=np.float64),
                "take.l1_sum": np.float64(l1.sum), "take.l1_avg": np.float64(l1.avg())})
    # the shortest take the differences allow
    del seen[:]
    al.load_pose(joints[:2].copy(), 0, 2, FPS, True)
    out["take2.vel"] = np.stack(seen, 1)
    # recover_from_ric, the reference's torch fp32
    ric = reference_ric()
    for name, (b, n, c, jn, s) in mr.RIC_CASES.items():
        out[f"ric.{name}"] = ric(torch.from_numpy(mr.ric_inputs(b, n, c, s)), jn).numpy()
    return out


def main():
    out = build()
    np.savez_compressed(os.path.join(HERE, "motion_metrics.npz"), **out)
    for k, v in out.items():
        print(f"{k:24s} {str(v.dtype):8s} {tuple(v.shape)}" + (f" {v}" if v.size == 1 else ""))
    print("beats per upper-body joint:", [int(out["take.beats"][:, i].sum()) for i in mr.UPPER_BODY])
    print("entries where the corrected rule differs:", int((out["take.beats"] != out["take.beats_corrected"]).sum()))
    print("bytes:", os.path.getsize(os.path.join(HERE, "motion_metrics.npz")))


if __name__ == "__main__":
    main()

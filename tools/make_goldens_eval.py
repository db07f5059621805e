#!/usr/bin/env python3
"""Generate tests/golden/eval_reference*.npz by running the REFERENCE's
utils/eval.py on the seeded cases of tests/eval_cases.py.

Build machine only: needs the reference checkout (REF below), like
tools/make_goldens.py.  utils/eval.py is loaded by file path; the one thing it
imports besides numpy, cv2, is not installed, so a stand-in module providing
only INTER_NEAREST and a numpy ``remap`` (tests/eval_cases.py; the rule is
docs/EVAL_SPEC.md's reading of OpenCV) is put in its place.  Nothing else of
the reference is restated for the run.  The ``evaluate`` case composes the
reference's two functions per frame the way utils/testing.py:64-93 does, with
the restated frame_generator / get_count_image of tests/eval_cases.py
(utils/testing.py itself cannot be imported: its .data needs a native module
that is absent).

Written (in parts of at most 950 000 bytes): inputs and reference outputs of
  prop_<HxW>_<dtype>_*    propagation, K = 6 maps, 5 frames, full frame
  err_<case>_*            flow_error_dense under the four is_car / is_dense variants
  eval_*                  per-frame and mean results of a 7-frame sequence
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
REF = Path('/root/reference')
OUT = REPO / 'tests' / 'golden'
LIMIT = 950_000      # bytes per part: headroom under the 1 MiB limit for a committed file

sys.path.insert(0, str(REPO))
from tests import eval_cases as ec  # noqa: E402


def save_parts(stem, arrays):
    """np.savez_compressed in parts of at most LIMIT bytes: <stem>.npz,
    <stem>.part2.npz, ... (tests/conftest.py merges them; the scheme of
    tools/make_goldens.py)."""
    import io

    def size(d):
        buf = io.BytesIO()
        np.savez_compressed(buf, **d)
        return buf.tell()
    parts = []
    for k in sorted(arrays, key=lambda k: -arrays[k].nbytes):
        for part in parts:
            if size(dict(part, **{k: arrays[k]})) <= LIMIT:
                part[k] = arrays[k]
                break
        else:
            parts.append({k: arrays[k]})
    for old in OUT.glob(f'{stem}.part*.npz'):
        old.unlink()
    for i, part in enumerate(parts):
        name = f'{stem}.npz' if i == 0 else f'{stem}.part{i + 1}.npz'
        np.savez_compressed(OUT / name, **part)
        print(name, (OUT / name).stat().st_size, 'bytes,', len(part), 'arrays')


def load_reference_eval():
    sys.modules['cv2'] = ec.cv2_standin()
    spec = importlib.util.spec_from_file_location('reference_utils_eval',
                                                  REF / 'utils' / 'eval.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recorded_steps(ref, x_maps, y_maps, ts, start, stop):
    """Run the reference's estimate_corresponding_gt_flow and record which map
    each of its prop_flow calls read and with which scale factor."""
    steps = []
    inner = ref.prop_flow

    def spy(x_flow, y_flow, xi, yi, xm, ym, scale_factor=1.0):
        k = [i for i in range(len(x_maps)) if np.shares_memory(x_flow, x_maps[i])]
        assert len(k) == 1
        steps.append((k[0], float(scale_factor)))
        return inner(x_flow, y_flow, xi, yi, xm, ym, scale_factor)
    ref.prop_flow = spy
    try:
        with np.errstate(invalid='ignore', over='ignore'):
            u, v = ref.estimate_corresponding_gt_flow(x_maps, y_maps, ts, start, stop)
    finally:
        ref.prop_flow = inner
    if steps:
        return u, v, 0, [s[0] for s in steps], [s[1] for s in steps]
    # direct scale: no prop_flow call; the map is the one the result is a multiple of
    dt, k = stop - start, int(np.searchsorted(ts, start, side='right')) - 1
    gt_dt = ts[k + 1] - ts[k]
    assert np.array_equal(u, x_maps[k] * dt / gt_dt, equal_nan=True)
    return u, v, 1, [k, k], [float(dt), float(gt_dt)]


def main():
    ref = load_reference_eval()
    out = {}

    # --- propagation -------------------------------------------------------
    out['prop_ts'] = ec.GT_TS
    out['prop_frames'] = np.array([f[1:] for f in ec.PROP_FRAMES])
    for si, shape in enumerate(ec.SHAPES):
        for dtype in (np.float32, np.float64):
            key = ec.prop_key(shape, dtype)
            xm, ym = ec.make_maps(shape, dtype, 100 + si)
            out[f'{key}_x'], out[f'{key}_y'] = xm, ym
            for f, (name, start, stop) in enumerate(ec.PROP_FRAMES):
                start, stop = np.float64(start), np.float64(stop)
                u, v, mode, maps, scales = recorded_steps(ref, xm, ym, ec.GT_TS, start, stop)
                out[f'{key}_u{f}'], out[f'{key}_v{f}'] = u, v
                if si == 0 and dtype == np.float32:
                    out[f'plan_mode{f}'] = np.array(mode)
                    out[f'plan_maps{f}'] = np.array(maps)
                    out[f'plan_scales{f}'] = np.array(scales, np.float64)
                print(key, name, 'mode', mode, maps, scales, u.dtype,
                      'non-finite', int((~np.isfinite(u)).sum() + (~np.isfinite(v)).sum()),
                      'masked', int((u == 0).sum()))

    # --- endpoint error ----------------------------------------------------
    for name, shape, seed, empty in ec.ERROR_CASES:
        gt, pred, count = ec.make_error_case(shape, seed, empty)
        out[f'err_{name}_gt'], out[f'err_{name}_pred'] = gt, pred
        out[f'err_{name}_count'] = count.astype(np.uint8)
        for vname, is_car, is_dense in ec.ERROR_VARIANTS:
            with np.errstate(invalid='ignore'), np.testing.suppress_warnings() as sup:
                sup.filter(RuntimeWarning)
                aee, pct, n = ref.flow_error_dense(gt, pred, count, is_car, is_dense)
            out[f'err_{name}_{vname}'] = np.array([aee, pct, n], np.float64)
            print('err', name, vname, aee, pct, n)

    # --- evaluate: utils/testing.py:64-93, composed ------------------------
    case = ec.make_eval_case()
    ev_crop, im_crop = ec.EventCrop(ec.EVAL_BOX), ec.ImageCrop(ec.EVAL_BOX)
    rows = []
    AEE_sum = percent_AEE_sum = 0       # the reference's running sums, types and all
    for i, (e, start, stop) in enumerate(ec.frame_generator(list(case['events']),
                                                            case['frames'])):
        e = ev_crop(np.array(e).T).T
        flow = case['flows'][i]
        with np.errstate(invalid='ignore', over='ignore'):
            u, v = ref.estimate_corresponding_gt_flow(case['x_maps'], case['y_maps'],
                                                      case['ts'], start, stop)
        gt_flow = im_crop(np.dstack((u, v)))
        count = ec.get_count_image(e, gt_flow.shape[:2])
        aee, pct, n = ref.flow_error_dense(gt_flow, flow, count, False)
        AEE_sum += aee
        percent_AEE_sum += pct
        rows.append([aee, pct, n, np.max(flow), np.min(flow)])
        print('eval frame', i, aee, pct, n)
    rows = np.array(rows, np.float64)
    out.update({f'eval_{k}': v for k, v in case.items()})
    out['eval_frame_results'] = rows
    out['eval_mean'] = np.array([float(AEE_sum) / len(rows), percent_AEE_sum / len(rows)])
    save_parts('eval_reference', out)


if __name__ == '__main__':
    main()

"""Child process of tests/test_gpu_avg_timestamp_pyramid_capture.py (a GPU fault
must not take the test runner down): one scenario of the captured step that
carries the average-timestamp term on every flow scale, printed as one JSON
line.  The loops, the batches and the audit are those of
tests/event_terms_capture_child.py.

  framed      RANGER, the term on every scale with three references and
              polarity, beside the frames' loss
  frameless   ADAM, batches without frames: the contrast term on the finest
              flow and the term on every scale beside the frameless loss

Either: train(capture=True, capture_event_terms=True, avg_timestamp_scales='all')
against train(capture=False) of an identical model, 5 optimizer steps of 2
micro-batches; the micro-batches from the seventh on bring more events than the
recorded buffers hold, so both roles are recorded a second time.
"""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from tests import event_terms_capture_child as base  # noqa: E402
from tests.capture_child import unique_pixel_batch  # noqa: E402

STEPS, ACCUM = 5, 2
# events per sample: 3072 a batch in buffers of 4096 (padded slots), then 5120, which they do not hold;
# the first micro-batch of the larger kind
SMALL, LARGE, GROWS_AT = 1536, 2560, 6
PYRAMID = ('avgts_pyramid_splat_kernel', 'avgts_pyramid_close_kernel', 'avgts_pyramid_bwd_events_kernel',
           'avgts_pyramid_bwd_close_kernel')
OPTIONS = {
    'framed': {'avg_timestamp_weight': 0.5, 'avg_timestamp_scales': 'all',
               'avg_timestamp_references': ('start', 'middle', 'end'), 'avg_timestamp_polarity': True},
    'frameless': {'contrast_weight': 0.25, 'avg_timestamp_weight': 0.5, 'avg_timestamp_scales': 'all'},
}


def scenario(name):
    base.KERNELS['avg_timestamp_pyramid'] = PYRAMID     # counted by the audit of run_loop beside the others
    args = base.parse('RANGER' if name == 'framed' else 'ADAM', STEPS, ACCUM)
    data = [unique_pixel_batch(11000 + i, base.B, base.H, base.W, SMALL if i < GROWS_AT else LARGE)
            for i in range(STEPS * ACCUM)]
    if name == 'frameless':
        data = [base.frameless(b) for b in data]
    opts = OPTIONS[name]
    eager = base.run_loop(args, data, 71, False, opts)
    cap = base.run_loop(args, data, 71, True, opts)
    e_rows, c_rows = eager['rows'], cap['rows']
    i = cap['info']
    levels = [r for r in c_rows if r[0].startswith('Train/avg timestamp/')]
    mean = [r for r in c_rows if r[0] == 'Train/avg timestamp']
    return {'rows_equal': e_rows == c_rows, 'n_rows': len(e_rows),
            'first_diff': next(((a, b) for a, b in zip(e_rows, c_rows) if a != b), None),
            'params_equal': base._same(eager['params'], cap['params']),
            'level_tags': sorted({r[0] for r in levels}), 'n_levels': len(levels), 'n_mean': len(mean),
            'levels_equal': levels == [r for r in e_rows if r[0].startswith('Train/avg timestamp/')],
            'mean_moves': len({r[1] for r in mean}) > 1,
            'n_contrast': len([r for r in c_rows if r[0] == 'Train/contrast']),
            'capture_lines': cap['capture_lines'] + eager['capture_lines'],
            'replays': i['replays'], 'roles': sorted(set(i['roles'])), 'failed': i['failed'],
            'recaptures': i['recaptures'], 'loops': i['loops'], 'unheld': i['unheld'],
            'ours_foreign': i['ours_foreign'], 'kernels': i['kernels'], 'stderr_tail': cap['stderr_tail']}


if __name__ == '__main__':
    os.environ.pop('DVSOF_LOOPBACK', None)
    print(json.dumps(scenario(sys.argv[1])), flush=True)

"""What the predictor computes and launches, as JSON lines: run it on two checkouts and
compare the files line by line (profiles/predictor_table/README.md).

  digest   bare Predictor, seeded weights / input / flow gradients, two consecutive eager
           forward + backward steps (the second accumulates into ``p.grad``): SHA-256 of
           the bytes of each of the 4 flows, the 32 ``p.grad`` and the input gradient, per
           operand mode, activation, shape, and: training on two streams, training with
           DVSOF_WGRAD_STREAM=0, inference under no_grad.  A step's line holds ONE SHA-256
           over those 37 digests in that order (a file of a few KB that can be committed);
           --per-tensor writes the 37 themselves, to find which tensor differs
  launch   the full model's captured training step, read from the step executor BEFORE
           its first replay (capture order, greedy lanes: functions of the graph alone):
           counts, the kernel names in order of first launch, and (lane, cross-lane
           waits, index of the name) per node

    python tools/predictor_trace.py --out FILE [--per-tensor]
"""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
from torch import nn  # noqa: E402

CONFIGS = (('f32', 'relu'), ('f32', 'mish'), ('bf16', 'relu'), ('bf16x3', 'relu'),
           ('bf16s', 'relu'), ('bf16s', 'mish'))
SHAPES = ((1, 5, 96, 160), (8, 5, 256, 256))


def sha(t):
    return hashlib.sha256(b'' if t is None else t.detach().cpu().numpy().tobytes()).hexdigest()


def digests(dtype, act, shape, mode, input_grad, per_tensor):
    from dvs_of_training_framework_amd.predictor import Predictor
    os.environ['DVSOF_WGRAD_STREAM'] = '0' if mode == 'train1' else '1'
    torch.manual_seed(11)
    net = Predictor(shape[1], nn.Mish() if act == 'mish' else nn.ReLU(), dtype).cuda()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(shape, generator=g).cuda().requires_grad_(input_grad)
    gflows = [torch.randn(shape[0], 2, shape[2] >> k, shape[3] >> k, generator=g).cuda()
              for k in (3, 2, 1, 0)]
    steps = []
    for _ in range(2):
        if mode == 'infer':
            with torch.no_grad():
                flows = net(x)
        else:
            flows = net(x)
            torch.autograd.backward(flows, gflows)
        torch.cuda.synchronize()
        each = [sha(f) for f in flows] + [sha(p.grad) for p in net.param_list()] + [sha(x.grad)]
        steps.append(each if per_tensor else hashlib.sha256(''.join(each).encode()).hexdigest())
    return steps


def launch_list(dtype):
    from dvs_of_training_framework_amd import synthetic
    from dvs_of_training_framework_amd.capture import CapturedTrainStep
    from dvs_of_training_framework_amd.loss import init_losses
    from dvs_of_training_framework_amd.net import Model
    from dvs_of_training_framework_amd.optim import FusedAdamW
    os.environ['DVSOF_WGRAD_STREAM'] = '1'
    B, H, W = 8, 256, 256
    torch.manual_seed(5)
    model = Model('cuda', event_representation_depth=5, compute_dtype=dtype)
    model.train()
    opt = FusedAdamW(model.predictor.parameters(), lr=1e-3, weight_decay=1e-4, amsgrad=True)
    ev = init_losses((H, W), B, model, 'cuda', sequence_length=1)
    batch = synthetic.to_torch(synthetic.make_batch(900, B, H, W, None), 'cuda')
    step = CapturedTrainStep(model, ev, opt, [0.5, 1, 1], 'cuda', batch, executor=True)
    x = step.executor
    nodes = x.nodes()
    names = list(dict.fromkeys(name for _, _, _, name in nodes))
    out = {'kernels': x.kernels, 'lanes': x.lanes, 'events': x.events, 'waits': x.waits,
           'marks': x.marks, 'names': names,
           'nodes': [(lane, nw, names.index(name)) for lane, _, nw, name in nodes]}
    torch.cuda.synchronize()
    step.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', required=True)
    ap.add_argument('--per-tensor', action='store_true')
    a = ap.parse_args()
    with open(a.out, 'w') as f:
        def emit(**row):
            f.write(json.dumps(row) + '\n')
            f.flush()
        for shape in SHAPES:
            for dtype, act in CONFIGS:
                for mode, input_grad in (('train2', False), ('train2', True), ('train1', False),
                                         ('train1', True), ('infer', False)):
                    emit(kind='digest', dtype=dtype, act=act, shape=shape, mode=mode,
                         input_grad=input_grad,
                         steps=digests(dtype, act, shape, mode, input_grad, a.per_tensor))
        for dtype in ('f32', 'bf16s'):
            emit(kind='launch', dtype=dtype, **launch_list(dtype))


if __name__ == '__main__':
    main()

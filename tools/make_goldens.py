#!/usr/bin/env python3
"""Generate tests/golden/* by running the REFERENCE next to seeded inputs.

Container-only: needs /root/reference (absent on the GPU box) and
/opt/conda/bin/h5dump (h5py is not installed).  Nothing of the reference's
source is copied; only data the reference's tests hold (HDF5 fixtures) and
numbers the reference computes are written out.

What is produced
  (the .npz sets are written in parts of at most 10^6 bytes: <name>.npz, <name>.part2.npz, ...)
  fixtures.npz        frames/events/timestamps of tests/data/seq/00000{0..9}.hdf5
                      and the (single, 10x duplicated) tests/data/pred flow
  loss_reference.npz  utils.loss.Losses outputs + autograd flow gradients on
                      the reference's three golden tests, the 10-fixture table
                      and seeded synthetic multi-scale cases
  plumbing.json       DummyNet / get_local_idx / process_minibatch witnesses
                      (config 1 of BASELINE.json) and LR-schedule sequences
"""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
REF = Path('/root/reference')
OUT = REPO / 'tests' / 'golden'
H5DUMP = '/opt/conda/bin/h5dump'

sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REF))

from dvs_of_training_framework_amd import synthetic  # noqa: E402
from utils.loss import Losses, init_losses  # noqa: E402  (reference)
from utils.timer import FakeTimer  # noqa: E402  (reference)
from utils.training import process_minibatch, combined_loss  # noqa: E402
from DummyNet.net import Model as DummyModel, get_local_idx  # noqa: E402


LIMIT = 10 ** 6      # bytes per committed file (under 1 MiB)


def save_parts(stem, arrays):
    """np.savez_compressed in parts of at most LIMIT bytes: <stem>.npz,
    <stem>.part2.npz, ... (tests/conftest.py merges them).  Largest arrays
    first, each into the first part it still fits in."""
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


def h5read(path, name, dtype, shape):
    with tempfile.NamedTemporaryFile(suffix='.bin') as tmp:
        subprocess.run([H5DUMP, '-d', name, '-b', 'LE', '-o', tmp.name,
                        str(path)], check=True, stdout=subprocess.DEVNULL)
        data = np.fromfile(tmp.name, dtype=dtype)
    return data.reshape(shape)


def extract_fixtures():
    seq = REF / 'tests' / 'data' / 'seq'
    pred = REF / 'tests' / 'data' / 'pred'
    out = {}
    frames, starts, stops = [], [], []
    for i in range(10):
        f = seq / f'{i:06d}.hdf5'
        im1 = h5read(f, 'image1', np.uint8, (260, 346))
        im2 = h5read(f, 'image2', np.uint8, (260, 346))
        ev = h5read(f, 'events', np.float64, (-1, 4))
        starts.append(h5read(f, 'start', np.float64, ())[()])
        stops.append(h5read(f, 'stop', np.float64, ())[()])
        if frames:
            assert (frames[-1] == im1).all(), 'fixtures are consecutive'
        else:
            frames.append(im1)
        frames.append(im2)
        out[f'events_{i}'] = ev
    flows = [h5read(pred / f'{i:06d}.hdf5', 'flow', np.float32, (260, 346, 2))
             for i in range(10)]
    for fl in flows[1:]:
        assert (fl == flows[0]).all(), 'all pred fixtures are identical'
    out['frames'] = np.stack(frames)            # [11,260,346] u8
    out['start'] = np.array(starts)
    out['stop'] = np.array(stops)
    out['pred_flow'] = flows[0]                 # [260,346,2] f32
    save_parts('fixtures', out)
    return out


def run_reference_losses(shapes, batch_size, flows, flow_ts, flow_sample_idx,
                         images, timestamps, sample_idx,
                         weights=(0.5, 1.0, 1.0)):
    """-> terms [3,K] f32, loss f32, grads (list of ndarrays)."""
    flows = [torch.from_numpy(np.ascontiguousarray(f)).requires_grad_(True)
             for f in flows]
    ev = Losses(shapes, batch_size, 'cpu')
    loss, terms = combined_loss(ev, flows,
                                torch.from_numpy(flow_ts),
                                torch.from_numpy(flow_sample_idx),
                                torch.from_numpy(images),
                                torch.from_numpy(timestamps),
                                torch.from_numpy(sample_idx),
                                None, weights=list(weights))
    grads = [None] * len(flows)
    if loss.requires_grad:
        loss.backward()
        grads = [f.grad.numpy().copy() for f in flows]
    t = np.array([[float(v.detach()) for v in term] for term in terms],
                 dtype=np.float64)
    return t, float(loss.detach()), grads


def fixture_case(fx, i, use_pred, H=246, W=340):
    im = fx['frames'][i:i + 2, :H, :W].astype(np.float32)[:, None]
    ts = np.array([0, fx['stop'][i] - fx['start'][i]], dtype=np.float32)
    flow = np.zeros((1, 2, H, W), np.float32)
    if use_pred:
        flow = np.ascontiguousarray(
            fx['pred_flow'][:H, :W].transpose(2, 0, 1)[None])
    return run_reference_losses([(H, W)], 1, [flow], ts.reshape(1, 2),
                                np.zeros(1, np.int64), im, ts,
                                np.zeros(2, np.int64))


SYNTH_CASES = {
    # name: (seed, B, H, W, shapes or None (=4 pyramid scales), sigma, seq)
    'cfg1_64': (11, 4, 64, 64, None, 1.0, 1),
    'cfg2_256': (12, 2, 256, 256, None, 3.0, 1),
    'odd_17x23': (13, 3, 17, 23, [(5, 7), (9, 12), (17, 23)], 2.0, 1),
    'seq3_32x48': (14, 2, 32, 48, None, 1.5, 3),
    'big_flow_40x24': (15, 2, 40, 24, [(10, 6), (40, 24)], 30.0, 1),
}


def synth_case(name):
    seed, B, H, W, shapes, sigma, seq = SYNTH_CASES[name]
    batch = synthetic.make_batch(seed, B, H, W, events_per_sample=0,
                                 seq_len=seq)
    shapes = shapes or synthetic.scale_shapes(H, W)
    flows = synthetic.make_flows(seed + 1000, B, shapes, sigma)
    if name == 'odd_17x23':
        for f in flows:
            f[1] = 0  # one sample without any out-of-border pixel
    ts = batch['timestamps'].reshape(B, seq + 1)
    pre = (seq - 1) // 2  # predicted element = middle one
    flow_ts = np.ascontiguousarray(ts[:, pre:pre + 2])
    fsi = np.arange(B, dtype=np.int64)
    return dict(shapes=shapes, B=B, flows=flows, flow_ts=flow_ts,
                flow_sample_idx=fsi, images=batch['images'],
                timestamps=batch['timestamps'],
                sample_idx=batch['sample_idx'])


def loss_goldens(fx):
    out = {}
    # tests/loss/test_loss.py:8-22
    z = np.zeros
    t, l, g = run_reference_losses(
        [(5, 6)], 1, [z((1, 2, 5, 6), np.float32)],
        np.array([[0, 0.4]], np.float32), z(1, np.int64),
        z((2, 1, 5, 6), np.float32), np.array([0, 0.4], np.float32),
        z(2, np.int64))
    out['no_changes_terms'] = t
    table_zero, table_pred = [], []
    for i in range(10):
        t0, _, _ = fixture_case(fx, i, False)
        t1, l1, g1 = fixture_case(fx, i, True)
        table_zero.append(t0[:, 0])
        table_pred.append(t1[:, 0])
        if i == 1:
            out['fixture1_pred_grad'] = g1[0]
            out['fixture1_pred_loss'] = np.float64(l1)
    out['fixture_zero_terms'] = np.array(table_zero)   # [10,3]
    out['fixture_pred_terms'] = np.array(table_pred)   # [10,3]
    for name in SYNTH_CASES:
        c = synth_case(name)
        t, l, g = run_reference_losses(
            c['shapes'], c['B'], c['flows'], c['flow_ts'],
            c['flow_sample_idx'], c['images'], c['timestamps'],
            c['sample_idx'])
        out[f'{name}_terms'] = t
        out[f'{name}_loss'] = np.float64(l)
        for k, gk in enumerate(g):
            out[f'{name}_grad{k}'] = gk
        print(name, 'terms', t.tolist(), 'loss', l)
    save_parts('loss_reference', out)


def lr_sequence(warmup, half_life, rs, steps, n):
    """Restates train_flownet.py:91-99 (the module itself is not importable:
    tensorboard/h5py are missing) through torch's own LambdaLR so that the
    stepping convention (factor(step) after `step` scheduler.step() calls)
    is the reference's."""
    representation_start = steps * rs

    def pred(step):
        if step < warmup:
            return step / warmup
        return 2 ** (-(step - warmup) / half_life)

    def rep(step):
        if step > representation_start:
            return pred(step)
        return 0

    p = [torch.nn.Parameter(torch.zeros(1)) for _ in range(2)]
    opt = torch.optim.SGD([{'params': [p[0]]}, {'params': [p[1]]}], lr=1.0)
    sch = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=[rep, pred])
    seq = []
    for _ in range(n):
        seq.append([g['lr'] for g in opt.param_groups])
        opt.step()
        sch.step()
    return seq


def plumbing():
    out = {}
    li, sizes = get_local_idx(torch.tensor([0, 0, 1, 1, 2, 1, 2, 2, 2]))
    out['get_local_idx'] = {'local_idx': li.tolist(),
                            'shard_sizes': sizes.tolist()}
    # config 1 of BASELINE.json: DummyNet, 64x64x3, batch 4, CPU
    batch = synthetic.to_torch(synthetic.make_batch(1234, 4, 64, 64))
    model = DummyModel('cpu')
    ev = init_losses((64, 64), 4, model, 'cpu', sequence_length=1)
    loss, terms, tags, extra = process_minibatch(
        model, batch, FakeTimer(), 'cpu', True, ev, [0.5, 1, 1],
        return_prediction=True)
    out['cfg1'] = {
        'loss': float(loss), 'requires_grad': bool(loss.requires_grad),
        'terms': [[v for v in t] for t in terms],
        'tags': list(tags),
        'shapes': [list(p.shape) for p in extra['prediction']],
        'flow_ts': extra['flow_ts'].tolist(),
        'flow_sample_idx': extra['flow_sample_idx'].tolist(),
        'num_parameters': sum(p.numel() for p in model.parameters())}
    # prefix/suffix element selection (DummyNet/net.py:70-78)
    m2 = DummyModel('cpu', prefix_length=1, suffix_length=1)
    ts = torch.arange(8, dtype=torch.float32) * 0.04
    si = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1])
    r = m2({}, ts, si, (16, 16))
    out['prefix1_suffix1'] = {'flow_ts': r[1].tolist(),
                              'flow_sample_idx': r[2].tolist()}
    out['lr_schedule'] = {
        'args': dict(warmup=4, half_life=8.0, rs=0.5, steps=12, n=16),
        'lrs': lr_sequence(4, 8.0, 0.5, 12, 16)}
    (OUT / 'plumbing.json').write_text(json.dumps(out, indent=1))


def main():
    OUT.mkdir(parents=True, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(4)
    fx = extract_fixtures()
    loss_goldens(fx)
    plumbing()
    print('written:', sorted(p.name for p in OUT.iterdir()))


if __name__ == '__main__':
    main()

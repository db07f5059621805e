#!/usr/bin/env python3
"""What a checkpoint costs the training thread, at the benchmark shape.

    python tools/checkpoint_bench.py [--optimizers adamw ranger] [--reps 5]

Model, optimizer and batches are optim_bench.py's replay leg (batch 8,
256x256x5, executor replay, update fused into the backward).  Three legs, in
alternating blocks of ONE run; one JSON line each:

  reference  the stall of ``torch.save({'model': state_dict(), 'optimizer':
             state_dict(), 'global_step': n}, file)`` on the training thread
             (what train_flownet.py ran after its last step before there was
             a serializer: this leg runs on any commit)
  async      ``Serializer.checkpoint_model`` on the device path: host time
             inside the call (the training thread's stall), the gather
             launch by HIP events with its bytes and its share of the 6.29 TB/s a
             float4 copy reaches on this part, the device-to-host copy, the
             writer thread's time
  loop       samples/s over --loop-steps steps with a checkpoint every
             --interval steps (async, plain) against none

A commit without dvs_of_training_framework_amd.serializer says which legs it
lacks and measures the rest.
"""
import argparse
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from optim_bench import B, Leg, say  # noqa: E402

COPY_PEAK = 6.29e12     # bytes/s, read + write, of a float4 copy kernel on the MI355X


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def reference_stall(leg, path, step):
    torch.cuda.synchronize()        # the loop has read its loss: the stream is drained
    t0 = time.perf_counter()
    torch.save({'model': leg.model.state_dict(), 'optimizer': leg.opt.state_dict(),
                'global_step': step}, path)
    return (time.perf_counter() - t0) * 1e3


def async_stall(leg, serializer, step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    serializer.checkpoint_model(leg.model, leg.opt, step)
    host_ms = (time.perf_counter() - t0) * 1e3
    serializer.wait()
    snap, timing = serializer._snap, serializer.timings[-1]
    pack_ms = snap.pack_start.elapsed_time(snap.packed)
    return dict(host_ms=host_ms, pack_ms=pack_ms, bytes=snap.bytes,
                pack_share=2 * snap.bytes / (pack_ms * 1e-3) / COPY_PEAK,
                copy_ms=snap.copy_start.elapsed_time(snap.copied),
                writer_wait_ms=timing['wait_s'] * 1e3, writer_write_ms=timing['write_s'] * 1e3)


def loop_block(leg, steps, interval, checkpoint):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(1, steps + 1):
        leg.step()
        if checkpoint is not None and i % interval == 0:
            checkpoint(i)
    torch.cuda.synchronize()
    return B * steps / (time.perf_counter() - t0)


def measure(a, optimizer):
    try:
        from dvs_of_training_framework_amd.serializer import Serializer
    except ImportError:
        Serializer = None
        say(what='checkpoint', optimizer=optimizer, leg='async', note='not measured: this commit '
            'has no dvs_of_training_framework_amd.serializer; the loop leg runs without it too')
    leg = Leg(optimizer, 'f32', True, True)
    leg.settle(a.warmup)
    out = Path(tempfile.mkdtemp(prefix='dvsof_ckpt_'))
    fast = Serializer(out / 'async', keep_checkpoints_max=1, permanent_checkpoint_interval=0) \
        if Serializer else None
    plain = Serializer(out / 'plain', keep_checkpoints_max=1, permanent_checkpoint_interval=0,
                       async_snapshot=False) if Serializer else None
    ref, fastr, plainr = [], [], []
    for r in range(a.reps + 1):         # the legs alternate; the first round is set-up
        for _ in range(a.between):
            leg.step()
        x = reference_stall(leg, out / 'reference.pt', r)
        for _ in range(a.between):
            leg.step()
        y = async_stall(leg, fast, r) if fast else None
        for _ in range(a.between):
            leg.step()
        z = None
        if plain:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plain.checkpoint_model(leg.model, leg.opt, r)
            z = (time.perf_counter() - t0) * 1e3
        if r:
            ref.append(x), fastr.append(y), plainr.append(z)
    say(what='checkpoint', optimizer=optimizer, leg='reference',
        stall_ms=round(median(ref), 3), runs_ms=[round(v, 3) for v in ref],
        file_bytes=(out / 'reference.pt').stat().st_size)
    if fast:
        keys = list(fastr[0])
        say(what='checkpoint', optimizer=optimizer, leg='async',
            **{k: round(median([r[k] for r in fastr]), 4) for k in keys},
            host_runs_ms=[round(r['host_ms'], 3) for r in fastr], stalls=fast.stalls)
        say(what='checkpoint', optimizer=optimizer, leg='plain',
            stall_ms=round(median(plainr), 3), runs_ms=[round(v, 3) for v in plainr])
    modes = {'none': None}
    if fast:
        modes['async'] = lambda i: fast.checkpoint_model(leg.model, leg.opt, i)
        modes['plain'] = lambda i: plain.checkpoint_model(leg.model, leg.opt, i)
    else:
        modes['reference'] = lambda i: reference_stall(leg, out / 'reference.pt', i)
    rates = {m: [] for m in modes}
    for _ in range(a.loop_blocks):
        for m, fn in modes.items():
            rates[m].append(loop_block(leg, a.loop_steps, a.interval, fn))
            if fast:
                fast.wait()
    for m, v in rates.items():
        say(what='checkpoint', optimizer=optimizer, leg='loop', mode=m, interval=a.interval,
            steps=a.loop_steps, samples_per_s=round(sum(v) / len(v), 1),
            blocks=[round(x, 1) for x in v])
    if fast:
        fast.close(), plain.close()
    leg.close()


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--optimizers', nargs='+', default=['adamw', 'ranger'],
                   choices=('adamw', 'ranger'))
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--between', type=int, default=10, help='training steps between two checkpoints')
    p.add_argument('--warmup', type=int, default=20)
    p.add_argument('--loop-steps', type=int, default=300)
    p.add_argument('--loop-blocks', type=int, default=2)
    p.add_argument('--interval', type=int, default=100)
    a = p.parse_args()
    for optimizer in a.optimizers:
        measure(a, optimizer)


if __name__ == '__main__':
    main()

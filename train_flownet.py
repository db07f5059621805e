#!/usr/bin/env python3
"""Training entry point with the reference's flags and wiring
(train_flownet.py:31-217): model plugin -> optimizer + LambdaLR ->
``init_losses`` -> ``train``.  Additions: one process per GPU under torchrun
(RCCL gradient all-reduce overlapped with backward), ``--synthetic`` and
``--sequence DIR`` (one recorded sequence kept on the device),
``--recording FILE`` (one event-only recording, no frames at all;
docs/FRAMELESS_SPEC.md),
``--visualization-period N`` (pictures of the predicted flow on the
validation data every N steps; docs/RENDER_SPEC.md).

Checkpoints, resume and validation are the reference's (:142-217) through this
package's ``serializer.Serializer`` and ``hooks``: a run continues from the
newest checkpoint of ``--model`` unless ``--do_not_continue``, with its
optimizer, schedulers and its position in the data stream
(docs/CHECKPOINT_SPEC.md).

The reference's HDF5 data pipeline and TensorBoard writer are outside this
build's scope: the pipeline is imported from the
reference tree (``utils.dataloader``) when this file is dropped into it;
otherwise ``--synthetic``, ``--sequence``, ``--recording`` or
``--preprocessed-dataset-path`` supply batches in the same wire format.
"""
import sys
from argparse import ArgumentParser
from pathlib import Path

import torch
import torch.optim as optim

from dvs_of_training_framework_amd import parallel, synthetic
from dvs_of_training_framework_amd.loss import init_losses
from dvs_of_training_framework_amd.model import init_model
from dvs_of_training_framework_amd.optim import FusedAdamW, FusedRAdam, \
    FusedRanger
from dvs_of_training_framework_amd.options import (
    add_train_arguments, add_preprocessed_dataset_arguments, avg_timestamp_keywords,
    guard_requested, resolve_step_guard, validate_train_args, window_kwargs)
from dvs_of_training_framework_amd.hooks import EvaluationHook, \
    SerializationHook, SharpnessHook, ValidationHook, VisualizationHook
from dvs_of_training_framework_amd.serializer import Serializer
from dvs_of_training_framework_amd.timer import EventTimer, FakeTimer
from dvs_of_training_framework_amd.training import HostGuard, \
    make_hook_periodic, train

script_dir = Path(__file__).resolve().parent


def parse_args(argv):
    parser = ArgumentParser()
    parser = add_train_arguments(parser)
    parser = add_preprocessed_dataset_arguments(parser)
    args = parser.parse_args(argv)
    args = resolve_step_guard(args, parser)
    args = validate_train_args(args)
    args.model.mkdir(exist_ok=True, parents=True)
    args.log_path = args.model / 'log'
    return args


def get_params2optimize(model):            # train_flownet.py:50-54
    if hasattr(model, 'quantization_layer'):
        return [{'params': model.quantization_layer.parameters()},
                {'params': model.predictor.parameters()}]
    return [{'params': model.parameters()}]


def construct_optimizer(args, params):     # train_flownet.py:57-75
    for g in params:
        g['params'] = list(g['params'])
    params = [g for g in params if g['params']]   # e.g. parameter-free voxeliser
    if args.optimizer == 'ADAM':
        on_gpu = all(p.is_cuda for g in params for p in g['params'])
        opt = FusedAdamW if on_gpu else optim.AdamW
        return opt(params, lr=args.lr, weight_decay=args.wdw, amsgrad=True)
    if args.optimizer in ('RADAM', 'RANGER'):
        # un-vendored submodules upstream (RAdam/, Ranger-Deep-Learning-
        # Optimizer/): fused HIP restatements of the published algorithms
        assert all(p.is_cuda for g in params for p in g['params']), \
            f'--optimizer {args.optimizer} runs on the HIP path only'
        opt = FusedRAdam if args.optimizer == 'RADAM' else FusedRanger
        return opt(params, lr=args.lr, weight_decay=args.wdw)
    assert hasattr(torch.optim, args.optimizer), 'Unknown optimizer type'
    return getattr(torch.optim, args.optimizer)(params, lr=args.lr,
                                                weight_decay=args.wdw)


def make_schedulers(args):                 # train_flownet.py:91-99
    representation_start = args.training_steps * args.rs

    def pred_scheduler(step):
        if step < args.num_warmup_steps:
            return step / args.num_warmup_steps
        return 2 ** (-(step - args.num_warmup_steps) / args.half_life)

    def repr_scheduler(step):
        if step > representation_start:
            return pred_scheduler(step)
        return 0
    return pred_scheduler, repr_scheduler


def construct_train_tools(args, model, passed_steps=0):   # :78-109
    is_splitted = hasattr(model, 'quantization_layer')
    if is_splitted:
        representation_params = [{
            'params': list(model.quantization_layer.parameters()),
            'weight_decay': args.wdw}]
        predictor_params = [{'params': list(model.predictor.parameters())}]
    else:
        representation_params = []
        predictor_params = [{'params': list(model.parameters()),
                             'weight_decay': args.wdw}]
    pred_scheduler, repr_scheduler = make_schedulers(args)
    groups = representation_params + predictor_params
    lambdas = [repr_scheduler] * len(representation_params) + \
        [pred_scheduler] * len(predictor_params)
    keep = [i for i, g in enumerate(groups) if g['params']]
    optimizer = construct_optimizer(args, [groups[i] for i in keep])
    scheduler = optim.lr_scheduler.LambdaLR(
        optimizer, lr_lambda=[lambdas[i] for i in keep])
    for _ in range(passed_steps):
        scheduler.step()
    return optimizer, scheduler


class SyntheticLoader:
    """Endless seeded batches in the reference's wire format
    (utils/dataset.py:961-1020), rank-sharded by seed."""

    def __init__(self, args, rank, steps, start=0, seed=1234):
        """``steps`` batches from batch ``start`` on: batch i is seeded by i,
        so a resumed run draws what the uninterrupted one would have."""
        self.args, self.rank, self.steps = args, rank, steps
        self.next, self.seed = int(start), seed

    def __len__(self):
        return self.steps

    def state(self):
        return {'next': int(self.next)}

    def restore(self, state):
        self.next = int(state['next'])

    def __iter__(self):
        a = self.args
        seq = a.prefix_length + a.suffix_length + 1
        for i in range(self.next, self.next + self.steps):
            self.next = i + 1
            yield synthetic.to_torch(synthetic.make_batch(
                self.seed + self.rank + 1000 * i, a.mbs, a.height, a.width,
                a.synthetic_events, seq_len=seq))


class _FixedBatches:
    """The same ``n`` seeded batches at every pass (validation)."""

    def __init__(self, args, n, seed):
        self.args, self.n, self.seed = args, n, seed

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(SyntheticLoader(self.args, 0, self.n, seed=self.seed))


# training batches are seeded 1234 + rank + 1000 * i: another residue class
VALIDATION_SEED = 1234 + 500


def preprocessed_position(samples_passed, world, rank, mbs):
    """Sample the preprocessed loader of ``rank`` continues from: every rank
    has passed ``samples_passed`` samples, ``_Strided`` then leaves out the
    other ranks' batches."""
    return samples_passed * world + rank * mbs


class _Strided:
    """Every rank takes one batch and skips the other ranks' (the loader is
    sequential and cyclic: rank r starts r batches in, set_index above)."""

    def __init__(self, loader, world):
        self.loader, self.world = loader, world

    def __iter__(self):
        return self

    def __next__(self):
        batch = next(self.loader)
        for _ in range(self.world - 1):
            next(self.loader)
        return batch


class _NullLogger:
    def add_scalar(self, *a, **k):
        pass


def make_logger(args, rank):
    if rank == 0:
        try:
            from torch.utils.tensorboard import SummaryWriter
            # (flushed by the serialization hook only, as in the reference)
            return SummaryWriter(str(args.log_path), max_queue=100000000,
                                 flush_secs=100000000)
        except Exception:       # tensorboard is not installed everywhere
            pass
    return _NullLogger()


def check_representation_args(args, world):
    """More than one process with a learnable representation needs the
    resident gradient slot: that is what joins the gradient exchange."""
    learn = getattr(args, 'learnable_representation', False)
    resident = getattr(args, 'representation_resident', False)
    if resident and not learn:
        raise SystemExit('--representation-resident needs --learnable-representation')
    if getattr(args, 'representation_deterministic', False) and not learn:
        raise SystemExit('--representation-deterministic needs --learnable-representation')
    if resident and torch.device(args.device).type != 'cuda':
        raise SystemExit('--representation-resident keeps the gradient of the knots in a '
                         f'device slot: it needs a GPU (--device {args.device})')
    if world > 1 and learn and not resident:
        raise SystemExit('--learnable-representation in more than one process needs '
                         '--representation-resident: only the resident gradient of the '
                         'knots is part of the gradient exchange')


def note(text):
    """One line on stderr (prefix ``run:``; ``capture:`` lines are the loop's)."""
    print(f'run: {text}', file=sys.stderr)


def make_train_loader(args, device, rank, world, steps, samples_passed):
    """The training loader for ``steps`` micro-batches, ``samples_passed``
    samples into the run (a loader with ``restore`` is positioned by the
    caller from its checkpointed state instead)."""
    if args.synthetic:
        return SyntheticLoader(args, rank, steps)
    if getattr(args, 'sequence', None) is not None:
        # one recorded sequence, resident on the device: batches are a window
        # table and one gather launch each (sequence.py); ranks draw different
        # permutations
        import numpy as np
        from dvs_of_training_framework_amd.sequence import FrameSequence, \
            SequenceLoader
        return SequenceLoader(
            FrameSequence.from_directory(args.sequence, device), args.shape,
            args.mbs, augmentation=True, collapse_length=args.cl,
            seq_length=args.prefix_length + args.suffix_length + 1,
            rng=np.random.default_rng(1234 + rank), steps=steps)
    if getattr(args, 'recording', None) is not None:
        # one event-only recording, resident on the device: windows cut from
        # the event stream, frameless batches (sequence.EventWindowLoader)
        import numpy as np
        from dvs_of_training_framework_amd.sequence import EventWindowLoader, \
            WindowedEvents
        return EventWindowLoader(
            WindowedEvents.from_file(args.recording, device=device, **window_kwargs(args)),
            args.shape, args.mbs, augmentation=True, collapse_length=args.cl,
            seq_length=args.prefix_length + args.suffix_length + 1,
            rng=np.random.default_rng(1234 + rank), steps=steps)
    if getattr(args, 'preprocessed_dataset_path', None) is not None:
        # utils/dataloader.py:89-100: the preprocessed (encoded / quantized)
        # dataset; --compact-events keeps raw events in their 9 B/event columns
        # all the way to the device voxeliser.  Ranks read disjoint strides.
        from dvs_of_training_framework_amd.preprocessed import \
            PreprocessedDataloader
        loader = PreprocessedDataloader(
            path=args.preprocessed_dataset_path, batch_size=args.mbs,
            is_raw=args.is_raw, cache_dir=getattr(args, 'cache_dir', None),
            cache_size=getattr(args, 'cache_size', 0),
            process_only_once=False,
            compact=getattr(args, 'compact_events', False))
        loader.set_index(preprocessed_position(samples_passed, world, rank,
                                               args.mbs))
        return _Strided(loader, world) if world > 1 else loader
    try:    # dropped into the reference tree: use its data pipeline
        from utils.dataloader import get_trainset_params, get_dataloader, \
            choose_data_path
        return get_dataloader(get_trainset_params(choose_data_path(args)),
                              sample_idx=samples_passed)
    except ImportError as e:
        raise SystemExit(
            'no dataset pipeline importable (the reference\'s utils.* and '
            f'h5py are needed: {e}); pass --synthetic') from e


def make_validation_loader(args, device):
    """None: nothing to validate on (said once on stderr)."""
    if getattr(args, 'validation_sequence', None) is not None:
        from dvs_of_training_framework_amd.sequence import FrameSequence, \
            SequenceLoader
        return SequenceLoader(
            FrameSequence.from_directory(args.validation_sequence, device),
            args.shape, args.mbs, augmentation=False,
            seq_length=args.prefix_length + args.suffix_length + 1, steps=None)
    if getattr(args, 'validation_recording', None) is not None:
        from dvs_of_training_framework_amd.sequence import EventWindowLoader, \
            WindowedEvents
        return EventWindowLoader(
            WindowedEvents.from_file(args.validation_recording, device=device,
                                     **window_kwargs(args)),
            args.shape, args.mbs, augmentation=False,
            seq_length=args.prefix_length + args.suffix_length + 1, steps=None)
    if args.synthetic and getattr(args, 'synthetic_validation_batches', 0) > 0:
        return _FixedBatches(args, args.synthetic_validation_batches,
                             VALIDATION_SEED)
    return None


def add_visualization(args, hooks, periodic, model, device, logger, losses, rank):
    """--visualization-period N > 0: a ``VisualizationHook`` on its own pass
    over the validation data every N optimizer steps.  0 constructs nothing."""
    if getattr(args, 'visualization_period', 0) <= 0:
        return
    loader = make_validation_loader(args, device)
    if loader is None:
        raise SystemExit('--visualization-period needs validation data '
                         '(--validation-sequence, or --synthetic-validation-batches '
                         'with --synthetic)')
    hooks['visualization'] = VisualizationHook(
        model, device, loader, logger, losses, args.loss_weights, args.is_raw, args,
        args.model / 'visualization', samples=args.visualization_samples, rank=rank)
    periodic['visualization'] = make_hook_periodic(hooks['visualization'],
                                                   args.visualization_period)


def add_evaluation(args, hooks, periodic, model, device, logger, rank):
    """--evaluation-period N > 0: an ``EvaluationHook`` every N optimizer steps
    (endpoint error against ground truth, and pictures).  0 constructs
    nothing.  Rank 0 alone holds the sequence and the ground truth."""
    if getattr(args, 'evaluation_period', 0) <= 0:
        return
    missing = [flag for flag, value in
               (('--validation-sequence', getattr(args, 'validation_sequence', None)),
                ('--validation-ground-truth', getattr(args, 'validation_ground_truth', None)))
               if value is None]
    if missing:
        raise SystemExit('--evaluation-period needs ' + ' and '.join(missing))
    sequence = gt = None
    if rank == 0:
        import numpy as np
        from dvs_of_training_framework_amd.sequence import FrameSequence
        sequence = FrameSequence.from_directory(args.validation_sequence, device)
        with np.load(str(args.validation_ground_truth)) as data:
            gt = {k: data[k] for k in ('timestamps', 'x_flow_dist', 'y_flow_dist')}
    hooks['evaluation'] = EvaluationHook(
        model, sequence, gt, logger, args.shape, args.model / 'evaluation',
        frame_step=args.evaluation_frame_step, pictures=args.evaluation_pictures,
        is_car=args.evaluation_is_car, rank=rank)
    periodic['evaluation'] = make_hook_periodic(hooks['evaluation'], args.evaluation_period)


def add_sharpness(args, hooks, periodic, model, device, logger, rank):
    """--sharpness-period N > 0: a ``SharpnessHook`` every N optimizer steps
    (flow warp loss of the validation sequence's own events, and pictures; no
    ground truth) at --sharpness-references, with --sharpness-polarity, and
    with --sharpness-rsat the ratio of squared average timestamps beside it.  0
    constructs nothing.  Rank 0 alone holds the sequence,
    and shares the one an ``EvaluationHook`` has already uploaded.  With
    --validation-recording the sequence is a ``WindowedEvents``: the hook needs
    the window boundaries and the events only."""
    if getattr(args, 'sharpness_period', 0) <= 0:
        return
    recording = getattr(args, 'validation_recording', None)
    if getattr(args, 'validation_sequence', None) is None and recording is None:
        raise SystemExit('--sharpness-period needs --validation-sequence or '
                         '--validation-recording')
    sequence = None
    if rank == 0:
        sequence = getattr(hooks.get('evaluation'), 'sequence', None)
        if sequence is None and recording is not None:
            from dvs_of_training_framework_amd.sequence import WindowedEvents
            sequence = WindowedEvents.from_file(recording, device=device, **window_kwargs(args))
        if sequence is None:
            from dvs_of_training_framework_amd.sequence import FrameSequence
            sequence = FrameSequence.from_directory(args.validation_sequence, device)
    hooks['sharpness'] = SharpnessHook(
        model, sequence, logger, args.shape, args.model / 'sharpness',
        frame_step=args.sharpness_frame_step, pictures=args.sharpness_pictures, rank=rank,
        references=getattr(args, 'sharpness_references', ('start',)),
        polarity=getattr(args, 'sharpness_polarity', False),
        **({'rsat': True} if getattr(args, 'sharpness_rsat', False) else {}))
    periodic['sharpness'] = make_hook_periodic(hooks['sharpness'], args.sharpness_period)


def restore_loader(loader, state, rank, world, global_step, args):
    """Position ``loader`` from the checkpoint's ``loader_state`` (a list
    indexed by rank); a checkpoint without one (the reference's) positions by
    the step count."""
    if not hasattr(loader, 'restore'):
        return
    states = state.get('loader_state')
    if states is not None and states[rank] is not None:
        loader.restore(states[rank])
    elif isinstance(loader, SyntheticLoader):
        loader.restore({'next': global_step * args.accum_step})


def check_resume_world(state, world, path):
    """A checkpoint holds one loader position per process that wrote it: a run
    of another size cannot continue its data stream."""
    written_by = state.get('world_size', 1)
    if written_by != world:
        raise SystemExit(
            f'{path} was written by {written_by} process(es), this run has '
            f'{world}: the position in the data stream does not carry over; '
            'pass --do_not_continue to start from step 0')


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    device = torch.device(args.device)
    rank, local, world = parallel.init_distributed(device.type)
    if device.type == 'cuda':
        device = torch.device('cuda', local if world > 1 else
                              (device.index or 0))
        torch.cuda.set_device(device)
    timers = EventTimer() if (args.timers and device.type == 'cuda') \
        else FakeTimer()

    check_representation_args(args, world)
    model = init_model(args, device)
    parallel.broadcast_parameters(model)

    serializer = Serializer(args.model, args.num_checkpoints,
                            args.permanent_interval,
                            async_snapshot=not getattr(args, 'sync_checkpoints',
                                                       False))
    known = serializer.list_known_steps()
    resume = not args.do_not_continue and len(known) > 0
    last_step = known[-1] if resume else 0
    optimizer, scheduler = construct_train_tools(args, model,
                                                 passed_steps=last_step)
    losses = init_losses(args.shape, args.mbs, model, device,
                         sequence_length=args.prefix_length +
                         args.suffix_length + 1, timers=timers)
    reducer = None
    if world > 1 and hasattr(model, 'predictor'):
        reducer = parallel.GradReducer()
        model.predictor.reducer = reducer

    logger = make_logger(args, rank)

    global_step, samples_passed, state = 0, 0, {}
    if resume:
        global_step, state = serializer.load_checkpoint(
            model, last_step, optimizer=optimizer, device=device)
        check_resume_world(state, world, serializer._id2path(last_step))
        samples_passed = state.pop('samples_passed', global_step * args.bs)
        note(f'continuing from step {global_step} ({samples_passed} samples)')
    remaining = max(args.training_steps - global_step, 0)

    loader = make_train_loader(args, device, rank, world,
                               remaining * args.accum_step, samples_passed)
    if resume:
        restore_loader(loader, state, rank, world, global_step, args)

    # the step guard (docs/STEP_GUARD_SPEC.md): on the device for the fused optimizers, a host
    # check in front of optimizer.step() for the others
    host_guard = None
    if guard_requested(args):
        skip = bool(getattr(args, 'skip_nonfinite_steps', False))
        if hasattr(optimizer, 'set_guard'):
            optimizer.set_guard(args.clip_grad_norm, skip)
        else:
            host_guard = HostGuard(args.clip_grad_norm, skip)

    oib = getattr(args, 'optimizer_in_backward', 'auto')
    if device.type == 'cuda' and hasattr(optimizer, 'fuse_into_backward') and \
            hasattr(model, 'predictor') and \
            (oib == 'on' or (oib == 'auto' and reducer is None and
                             getattr(args, 'compute_dtype', 'f32') == 'f32')):
        optimizer.fuse_into_backward(model.predictor)
    if getattr(args, 'device_feeder', False) and device.type == 'cuda' and args.is_raw:
        from dvs_of_training_framework_amd.feed import DeviceFeeder
        loader = DeviceFeeder(loader, device)

    def extra_state():
        extra = {'world_size': world}
        if hasattr(loader, 'state'):
            extra['loader_state'] = loader.state()
        return extra
    hooks = {'serialization': SerializationHook(serializer, model, optimizer,
                                                logger, extra_state, rank=rank)}
    periodic = {'serialization': make_hook_periodic(
        hooks['serialization'], args.checkpointing_interval)}
    validation_loader = None if args.skip_validation else \
        make_validation_loader(args, device)
    if validation_loader is not None:
        hooks['validation'] = ValidationHook(
            model, device, validation_loader, logger, losses,
            args.loss_weights, args.is_raw,
            **({'contrast_weight': args.contrast_weight,
                'contrast_references': getattr(args, 'contrast_references', ('start',)),
                'contrast_polarity': getattr(args, 'contrast_polarity', False),
                'contrast_scales': getattr(args, 'contrast_scales', 'finest')}
               if getattr(args, 'contrast_weight', 0.0) else {}),
            **avg_timestamp_keywords(args))
        periodic['validation'] = make_hook_periodic(hooks['validation'], args.vp)
    elif not args.skip_validation:
        note('no validation data (--validation-sequence, --validation-recording, or '
             '--synthetic-validation-batches with --synthetic): validation is skipped')
    add_visualization(args, hooks, periodic, model, device, logger, losses, rank)
    add_evaluation(args, hooks, periodic, model, device, logger, rank)
    add_sharpness(args, hooks, periodic, model, device, logger, rank)

    try:
        if not resume:
            hooks['serialization'](0, 0)
        if remaining > 0:
            if 'validation' in hooks:
                hooks['validation'](global_step, samples_passed)
            train(model, device, loader, optimizer, args.training_steps,
                  scheduler=scheduler, evaluator=losses, logger=logger,
                  weights=args.loss_weights, is_raw=args.is_raw,
                  accumulation_steps=args.accum_step, timers=timers,
                  hooks=periodic, init_step=global_step,
                  init_samples_passed=samples_passed,
                  max_events_per_batch=args.max_events_per_batch,
                  reducer=reducer, capture=getattr(args, 'capture', False),
                  guard=host_guard,
                  max_skipped_steps=getattr(args, 'max_skipped_steps', 32),
                  guard_agreement_every=args.checkpointing_interval,
                  contrast_weight=getattr(args, 'contrast_weight', 0.0),
                  contrast_references=getattr(args, 'contrast_references', ('start',)),
                  contrast_polarity=getattr(args, 'contrast_polarity', False),
                  contrast_scales=getattr(args, 'contrast_scales', 'finest'),
                  **avg_timestamp_keywords(args),
                  **({'capture_event_terms': True}
                     if getattr(args, 'capture_event_terms', False) else {}))
            samples = samples_passed + remaining * args.bs
            if args.training_steps % args.checkpointing_interval != 0:
                # (otherwise the periodic hook has just written this step)
                hooks['serialization'](args.training_steps, samples)
            if 'validation' in hooks:
                hooks['validation'](args.training_steps, samples)
        else:
            note(f'step {global_step} of {args.training_steps} is on disk: nothing to train')
    finally:
        if reducer is not None:
            reducer.close()
        serializer.close()


if __name__ == '__main__':
    main()

"""Command-line flags of the training entry point, restated 1:1 from the
reference (utils/options.py:10-347) so existing launch scripts keep working;
``--world-size`` / ``--synthetic*`` are additions for the MI355X build.
The reference module itself cannot be imported here (it imports the absent
``mish`` submodule at :7)."""
import argparse
import os
from pathlib import Path

import torch
import torch.nn as nn


class Mish(nn.Module):
    """x * tanh(softplus(x)) (Misra 2019) -- stands in for the un-vendored
    ``mish.mish.Mish`` (utils/options.py:7); the HIP conv stack fuses it."""

    def forward(self, x):
        return nn.functional.mish(x)


def add_common_arguments(parser):          # utils/options.py:10-19
    parser.add_argument('--allow-obsolete-code', action='store_true')
    parser.add_argument('--allow-arguments-change', action='store_true')
    return parser


def add_model_arguments(parser):           # utils/options.py:22-56
    parser.add_argument('--flownet_path', default=Path('EV_FlowNet'),
                        type=Path, required=False,
                        help='relative path to a model to train')
    parser.add_argument('--mish', action='store_true')
    parser.add_argument('-d', '--device', default=torch.device('cuda:0'),
                        type=torch.device, required=False)
    parser.add_argument('-bs', '--batch_size', dest='bs', default=32,
                        type=int, required=False,
                        help='batch size for an optimizer step')
    parser.add_argument('--profiling', choices=['CPU', 'NVTX', 'None'],
                        default='None')
    parser.add_argument('-sp', '--starting_point', dest='sp', default=None,
                        required=False)
    return parser


def add_dataset_arguments(parser):         # utils/options.py:59-113
    parser.add_argument('--ev_images', action='store_true')
    parser.add_argument('-cl', '--collapse_length', dest='cl', default=6,
                        type=int, required=False)
    parser.add_argument('--height', dest='height', default=256, type=int)
    parser.add_argument('--width', dest='width', default=256, type=int)
    parser.add_argument('--min-sequence-length', dest='min_sequence_length',
                        default=1, type=int)
    parser.add_argument('--max-sequence-length', dest='max_sequence_length',
                        default=1, type=int)
    parser.add_argument('--prefix-length', dest='prefix_length', default=0,
                        type=int)
    parser.add_argument('--suffix-length', dest='suffix_length', default=0,
                        type=int)
    parser.add_argument('--dynamic-sample-length',
                        dest='dynamic_sample_length', action='store_true')
    parser.add_argument('--event-representation-depth',
                        dest='event_representation_depth', default=9,
                        type=int)
    return parser


def add_dataloader_arguments(parser):      # utils/options.py:116-129
    parser.add_argument('-mbs', '--micro_batch_size', dest='mbs', default=32,
                        type=int, required=False,
                        help='batch size for a single forward-backward pass')
    parser.add_argument('--num_workers', dest='num_workers',
                        default=len(os.sched_getaffinity(0)), type=int)
    return parser


def add_preprocessed_dataset_arguments(parser):   # utils/options.py:150-173
    parser.add_argument('--preprocessed-dataset-path',
                        dest='preprocessed_dataset_path', default=None,
                        type=Path)
    parser.add_argument('--cache-dir', dest='cache_dir', default=None,
                        type=Path)
    parser.add_argument('--cache-size', dest='cache_size', default=5,
                        type=int)
    parser.add_argument('--process-only-once', dest='process_only_once',
                        action='store_true')
    return parser


def add_train_arguments(parser):           # utils/options.py:204-302
    parser = add_common_arguments(parser)
    parser = add_model_arguments(parser)
    parser = add_dataset_arguments(parser)
    parser = add_dataloader_arguments(parser)
    parser.add_argument('-m', '--model', required=True, type=Path,
                        help='Directory to store learned weights')
    parser.add_argument('--half_life', dest='half_life', default=100000,
                        type=float)
    parser.add_argument('-wdw', '--weight_decay_weight', dest='wdw',
                        default=1e-4, type=float)
    parser.add_argument('-ne', '--num_training_steps', dest='training_steps',
                        default=1000000, type=int)
    parser.add_argument('--num-warmup-steps', dest='num_warmup_steps',
                        default=0, type=int)
    parser.add_argument('-lr', '--learning_rate', dest='lr', default=1e-3,
                        type=float)
    parser.add_argument('-vp', '--validation_period', dest='vp', default=1000,
                        type=int)
    parser.add_argument('--optimizer', default='RANGER',
                        choices=['ADAM', 'RADAM', 'RANGER'])
    parser.add_argument('--loss_weights', default=[0.5, 1, 1], nargs=3,
                        type=float)
    parser.add_argument('--representation-start', dest='rs', default=0.5,
                        type=float)
    parser.add_argument('--num_checkpoints', dest='num_checkpoints',
                        default=2, type=int)
    parser.add_argument('--permanent_interval', dest='permanent_interval',
                        default=10000, type=int)
    parser.add_argument('--checkpointing_interval',
                        dest='checkpointing_interval', default=1000, type=int)
    parser.add_argument('--timers', dest='timers', action='store_true')
    parser.add_argument('--do_not_continue', dest='do_not_continue',
                        action='store_true')
    parser.add_argument('--max-events-per-batch', dest='max_events_per_batch',
                        default=35000000, type=int)
    parser.add_argument('--skip-validation', dest='skip_validation',
                        action='store_true')
    # --- additions of this build
    parser.add_argument('--compute-dtype', dest='compute_dtype', default='f32',
                        choices=['f32', 'bf16x3', 'bf16', 'bf16s'],
                        help='matrix-core operand type of the conv stack: exact f32, '
                             'bf16 hi+lo split (three products, ~f32 accuracy), bf16 '
                             '(operands rounded in registers; storage and accumulation '
                             'f32) or bf16s (bf16 twins of activations / gradients / '
                             'weight forms streamed through LDS; master weights, '
                             'gradients of weights and optimizer state stay f32)')
    parser.add_argument('--learnable-representation',
                        dest='learnable_representation', action='store_true',
                        help='learn the temporal kernel of the event representation '
                             '(docs/LEARNED_VOXEL_SPEC.md: a piecewise-linear lookup '
                             'table, initialised to the fixed voxel grid; it gets its '
                             'own parameter group, whose learning rate stays 0 until '
                             '--representation-start of the training steps)')
    parser.add_argument('--representation-radius', dest='representation_radius',
                        default=2, type=int, choices=[1, 2, 3],
                        help='support of the learnable kernel in bins')
    parser.add_argument('--representation-knots', dest='representation_knots',
                        default=8, type=int, choices=list(range(1, 17)),
                        help='knots per bin of the learnable kernel')
    parser.add_argument('--representation-resident',
                        dest='representation_resident', action='store_true',
                        help='with --learnable-representation: keep the gradient of '
                             'the knots in a persistent device slot '
                             '(net.LearnedVoxelGrid.make_resident).  Needed for '
                             '--capture to replay such a model and for more than one '
                             'process (the knots then join the gradient exchange); '
                             'the learned forward sums with float atomics, so a '
                             'replayed step equals its eager twin bit for bit only '
                             'where no voxel receives two events -- or, with '
                             '--representation-deterministic, on every input')
    parser.add_argument('--representation-deterministic',
                        dest='representation_deterministic', action='store_true',
                        help='with --learnable-representation: every forward of the '
                             'layer sums in 64-bit fixed point '
                             '(dvsof_learned_voxelize_tiled; docs/LEARNED_VOXEL_SPEC.md, '
                             'Order-independent forward) instead of with float '
                             'atomics: the same events give the same bits in any '
                             'order, so two runs from one seed agree bit for bit')
    parser.add_argument('--capture', action='store_true',
                        help='replay the loop body from one C call per micro-batch '
                             'once a batch signature has been seen (capture.CapturedLoop '
                             '/ the step executor; ADAM; with or without gradient '
                             'accumulation, with or without data parallelism -- the '
                             'executor then issues the gradient exchange; a run with '
                             '--contrast-weight or --avg-timestamp-weight is replayed '
                             'with --capture-event-terms, and runs eagerly without it)')
    parser.add_argument('--optimizer-in-backward', dest='optimizer_in_backward',
                        default='auto', choices=['auto', 'on', 'off'],
                        help='(auto resolves to off, and on is an error, with '
                             '--clip-grad-norm or --skip-nonfinite-steps: a bucket '
                             'updated during the backward cannot wait for the global '
                             'norm)  update a gradient bucket\'s parameters as soon as its '
                             'gradients are final (behind its all-reduce under data '
                             'parallelism) instead of in optimizer.step() '
                             '(optim.fuse_into_backward; same arithmetic).  auto: on '
                             'for --compute-dtype f32 in a single process, where the '
                             'HBM-bound update hides beside matrix-bound kernels '
                             '(+1.5 %%); off for the bf16 modes, which are '
                             'bandwidth-bound themselves, and under data parallelism '
                             '(the per-bucket waits for the exchange cost more than '
                             'the overlap gives: measured in a 1-rank group)')
    parser.add_argument('--clip-grad-norm', dest='clip_grad_norm', default=None,
                        type=float,
                        help='clip the global gradient norm of every optimizer step to '
                             'this value (clip_grad_norm_ semantics over all parameter '
                             'groups; docs/STEP_GUARD_SPEC.md).  With the fused '
                             'optimizers the norm is reduced and applied on the device, '
                             'inside the (captured) step; default: off')
    parser.add_argument('--skip-nonfinite-steps', dest='skip_nonfinite_steps',
                        action='store_true',
                        help='an optimizer step whose gradients hold a NaN or an Inf '
                             'writes nothing: no parameter, no optimizer state (the step '
                             'count and the schedule advance all the same); default: off')
    parser.add_argument('--max-skipped-steps', dest='max_skipped_steps', default=32,
                        type=int,
                        help='with --skip-nonfinite-steps: end the run once this many '
                             'optimizer steps IN A ROW were skipped (a policy value, '
                             'seen at logging steps)')
    parser.add_argument('--device-feeder', dest='device_feeder', action='store_true',
                        help='move batches to the device on a copy stream, one step '
                             'ahead (feed.DeviceFeeder), instead of tensor.to(device) '
                             'at the top of every step (utils/training.py:45-56)')
    parser.add_argument('--compact-events', dest='compact_events',
                        action='store_true',
                        help='with --preprocessed-dataset-path: hand raw '
                             'events to the device voxeliser in their 9 B/event '
                             'encoded columns (no int64 wire columns)')
    parser.add_argument('--sequence', dest='sequence', default=None, type=Path,
                        help='train from ONE recorded sequence kept on the device: a '
                             'directory of the per-frame <number>.hdf5 files (events, '
                             'image1, image2, start, stop); batches are cut by '
                             'sequence.SequenceLoader (collapse length -cl, sequence '
                             'length prefix + suffix + 1, random flip / rotation / crop '
                             'to --height x --width)')
    parser.add_argument('--synthetic', action='store_true',
                        help='train on seeded synthetic batches (no dataset)')
    parser.add_argument('--synthetic-events', dest='synthetic_events',
                        default=None, type=int,
                        help='events per synthetic sample (default H*W)')
    parser.add_argument('--validation-sequence', dest='validation_sequence',
                        default=None, type=Path,
                        help='validate (before and after training and every '
                             '--validation_period steps) on ONE recorded sequence, a '
                             'directory as for --sequence: one pass, central crop, no '
                             'augmentation')
    parser.add_argument('--synthetic-validation-batches',
                        dest='synthetic_validation_batches', default=0, type=int,
                        help='with --synthetic: validate on this many seeded batches '
                             '(seeds disjoint from the training batches\')')
    parser.add_argument('--visualization-period', dest='visualization_period',
                        default=0, type=int,
                        help='every this many optimizer steps render the first '
                             '--visualization-samples samples of the validation data '
                             '(frames on top, the predicted flow pyramid below; '
                             'docs/RENDER_SPEC.md) into <model>/visualization/step_N/ and, '
                             'where the logger takes images, into the log; 0: off')
    parser.add_argument('--visualization-samples', dest='visualization_samples',
                        default=4, type=int)
    parser.add_argument('--validation-ground-truth', dest='validation_ground_truth',
                        default=None, type=Path,
                        help='ground-truth flow of --validation-sequence: an MVSEC '
                             '*_gt_flow_dist.npz (timestamps, x_flow_dist, y_flow_dist) on '
                             'the clock of the sequence\'s image timestamps')
    parser.add_argument('--evaluation-period', dest='evaluation_period', default=0,
                        type=int,
                        help='every this many optimizer steps measure the endpoint error '
                             'of the live weights on --validation-sequence against '
                             '--validation-ground-truth (central crop to --height x '
                             '--width), log Evaluation/mean AEE and Evaluation/mean %%AEE '
                             'and draw --evaluation-pictures frames (events | prediction '
                             '| ground truth | endpoint error; docs/EVAL_PANELS_SPEC.md) '
                             'into <model>/evaluation/step_N/; 0: off')
    parser.add_argument('--evaluation-frame-step', dest='evaluation_frame_step',
                        default=1, type=int,
                        help='images a frame of the evaluation spans (the step of the '
                             'reference\'s test grid)')
    parser.add_argument('--evaluation-pictures', dest='evaluation_pictures', default=4,
                        type=int)
    parser.add_argument('--evaluation-is-car', dest='evaluation_is_car',
                        action='store_true',
                        help='outdoor driving sequence: rows from 190 on (the hood) are '
                             'not counted')
    parser.add_argument('--sharpness-period', dest='sharpness_period', default=0,
                        type=int,
                        help='every this many optimizer steps measure, without ground truth, '
                             'whether the flow of the live weights sharpens the events of '
                             '--validation-sequence (central crop to --height x --width): '
                             'log Sharpness/mean FWL (flow warp loss: variance of the image '
                             'of warped events over that of the count image, > 1 is '
                             'sharper), Sharpness/mean kept mass and Sharpness/frames '
                             'without events, and draw --sharpness-pictures frames (count '
                             'image | image of warped events; docs/IWE_SPEC.md) into '
                             '<model>/sharpness/step_N/; 0: off')
    parser.add_argument('--sharpness-frame-step', dest='sharpness_frame_step',
                        default=1, type=int,
                        help='images a frame of the sharpness measurement spans')
    parser.add_argument('--sharpness-pictures', dest='sharpness_pictures', default=4,
                        type=int)
    parser.add_argument('--sharpness-references', dest='sharpness_references',
                        default='start', type=str,
                        help='comma-separated reference times of the sharpness measurement, '
                             'among start, middle, end (any order, none twice): the events '
                             'are warped to each of these times of their frame, every image '
                             'has a flow warp loss of its own, Sharpness/mean FWL is their '
                             'mean and Sharpness/mean FWL/<reference> the mean per reference '
                             '(a collapsing flow is rewarded at the start and not at the '
                             'end; docs/IWE_SPEC.md section 8).  Needs --sharpness-period')
    parser.add_argument('--sharpness-polarity', dest='sharpness_polarity',
                        action='store_true',
                        help='accumulate ON and OFF events in images of their own in the '
                             'sharpness measurement, and log Sharpness/mean FWL/ON and /OFF.  '
                             'Needs --sharpness-period')
    parser.add_argument('--sharpness-rsat', dest='sharpness_rsat',
                        default=argparse.SUPPRESS, action='store_true',
                        help='beside the flow warp loss, log Sharpness/mean RSAT (ratio of the '
                             'squared average timestamps of the warped events over those at '
                             'zero flow: 1 at zero flow, below 1 where the flow aligns the '
                             'events of an edge, never below 0, so a collapsing flow is not '
                             'rewarded as it is by the FWL), from one splat for both, and draw '
                             'the average-timestamp images beside the two the pictures have '
                             '(docs/IWE_SPEC.md section 14).  Needs --sharpness-period')
    parser.add_argument('--contrast-weight', dest='contrast_weight', default=0.0,
                        type=float,
                        help='add this times the contrast-maximisation term to the '
                             'training loss: per prediction 1 - variance of the image of '
                             'the events warped along the finest flow / variance of their '
                             'count image, negative where the flow sharpens the events '
                             '(docs/CONTRAST_SPEC.md); logged as Train/contrast and '
                             'Validation/contrast.  Needs the raw events in their wire '
                             'columns on the device (not --ev_images; --compact-events only '
                             'with --compact-event-terms); --capture replays such a run only with '
                             '--capture-event-terms.  0: off')
    parser.add_argument('--contrast-references', dest='contrast_references',
                        default='start', type=str,
                        help='comma-separated reference times of the contrast term, among '
                             'start, middle, end (any order, none twice): the events are '
                             'warped to each of these times of their window and the term is '
                             'the mean over the images (Zhu et al. 2019: start,end; Shiba et '
                             'al. 2022: start,middle,end).  Needs --contrast-weight')
    parser.add_argument('--contrast-polarity', dest='contrast_polarity',
                        action='store_true',
                        help='accumulate ON and OFF events in images of their own in the '
                             'contrast term.  Needs --contrast-weight')
    parser.add_argument('--contrast-scales', dest='contrast_scales',
                        default=argparse.SUPPRESS, choices=('finest', 'all'),
                        help='the flow scales the contrast term is taken on: finest (the '
                             'default) supervises the finest flow alone; all takes the term of '
                             'every flow head on the events quantised to that head\'s grid, each '
                             'level weighing --contrast-weight / K, and logs Train/contrast/<tag> '
                             'per level beside the mean (docs/CONTRAST_SPEC.md sections 19-23).  '
                             'Needs --contrast-weight')
    parser.add_argument('--avg-timestamp-weight', dest='avg_timestamp_weight',
                        default=argparse.SUPPRESS, type=float,
                        help='add this times the average-timestamp term to the training '
                             'loss: per prediction the mean squared per-pixel average of the '
                             'distance in time between the events warped along the finest '
                             'flow and the reference time, over the same at zero flow: 1 at '
                             'zero flow, below 1 where the flow aligns the events of an edge '
                             '(docs/AVG_TIMESTAMP_SPEC.md; Zhu et al. 2019); logged as '
                             'Train/avg timestamp and Validation/avg timestamp.  With or '
                             'without --contrast-weight.  Needs the raw events in their wire '
                             'columns on the device (not --ev_images; --compact-events only with '
                             '--compact-event-terms); --capture replays such a run only with '
                             '--capture-event-terms.  Absent or 0: '
                             'off')
    parser.add_argument('--avg-timestamp-references', dest='avg_timestamp_references',
                        default=argparse.SUPPRESS, type=str,
                        help='comma-separated reference times of the average-timestamp term, '
                             'among start, middle, end (any order, none twice; default '
                             'start,end).  Needs --avg-timestamp-weight')
    parser.add_argument('--avg-timestamp-polarity', dest='avg_timestamp_polarity',
                        default=argparse.SUPPRESS, action='store_true',
                        help='accumulate ON and OFF events in images of their own in the '
                             'average-timestamp term.  Needs --avg-timestamp-weight')
    parser.add_argument('--avg-timestamp-scales', dest='avg_timestamp_scales',
                        default=argparse.SUPPRESS, choices=('finest', 'all'),
                        help='the flow scales the average-timestamp term is taken on: finest '
                             '(the default) supervises the finest flow alone; all takes the term '
                             'of every flow head on the events quantised to that head\'s grid, '
                             'each level weighing --avg-timestamp-weight / K, and logs Train/avg '
                             'timestamp/<tag> per level beside the mean '
                             '(docs/AVG_TIMESTAMP_SPEC.md sections 11-15).  Needs '
                             '--avg-timestamp-weight')
    parser.add_argument('--capture-event-terms', dest='capture_event_terms',
                        default=argparse.SUPPRESS, action='store_true',
                        help='with --capture and a positive --contrast-weight or '
                             '--avg-timestamp-weight: the captured step carries those terms, '
                             'with all their options, and the frameless batches of --recording, '
                             'instead of running the loop eagerly for them; bit-identical to '
                             'the eager step.  Opt-in: without it --capture decides as before')
    parser.add_argument('--compact-event-terms', dest='compact_event_terms',
                        default=argparse.SUPPRESS, action='store_true',
                        help='with --compact-events and a positive --contrast-weight or '
                             '--avg-timestamp-weight: those terms read the 9 B/event encoded '
                             'columns as they are (include/dvsof_event_terms_encoded.h), with all '
                             'their options, and give the bytes they give on the decoded wire '
                             'columns.  Opt-in: without it the terms refuse --compact-events as '
                             'before')
    parser.add_argument('--recording', dest='recording', default=None, type=Path,
                        help='train from ONE event-only recording kept on the device: a '
                             '.npz or .hdf5 file with the arrays x, y, t, p (sorted by t) and '
                             'shape = (H, W); no frames are needed or read '
                             '(docs/FRAMELESS_SPEC.md).  Windows are cut by --window-duration '
                             'or --window-events, batches by sequence.EventWindowLoader (the '
                             'rules of --sequence), and the loss is smoothness + out-of-border '
                             '+ the contrast-maximisation term: needs --contrast-weight > 0')
    parser.add_argument('--validation-recording', dest='validation_recording', default=None,
                        type=Path,
                        help='validate on ONE event-only recording, a file as for --recording '
                             '(one pass, central crop, no augmentation; the windows of '
                             '--window-duration / --window-events); --sharpness-period takes '
                             'it in place of --validation-sequence')
    parser.add_argument('--window-duration', dest='window_duration', default=None, type=float,
                        help='with --recording / --validation-recording: windows of this many '
                             'seconds from the first event on')
    parser.add_argument('--window-events', dest='window_events', default=None, type=int,
                        help='with --recording / --validation-recording: windows of this many '
                             'events (exactly one of --window-duration and --window-events)')
    parser.add_argument('--sync-checkpoints', dest='sync_checkpoints',
                        action='store_true',
                        help='write checkpoints on the training thread (state_dict() + '
                             'torch.save, the reference\'s way) instead of snapshotting '
                             'the device state in one launch and writing the file from '
                             'a writer thread (docs/CHECKPOINT_SPEC.md)')
    return parser


def validate_dataset_args(args):           # utils/options.py:305-309
    args.is_raw = not args.ev_images
    args.shape = (args.height, args.width)
    assert args.prefix_length + args.suffix_length < args.max_sequence_length
    return args


def guard_requested(args):
    return getattr(args, 'clip_grad_norm', None) is not None or \
        bool(getattr(args, 'skip_nonfinite_steps', False))


def resolve_step_guard(args, parser=None):
    """--optimizer-in-backward against the step guard: ``auto`` resolves to
    ``off`` when a guard is requested, an explicit ``on`` is an argparse
    error (``parser.error``; SystemExit without a parser)."""
    if not guard_requested(args):
        return args
    clip = args.clip_grad_norm

    def fail(message):
        if parser is not None:
            parser.error(message)
        raise SystemExit(message)
    if clip is not None and not clip > 0:
        fail(f'--clip-grad-norm must be positive, got {clip}')
    if getattr(args, 'max_skipped_steps', 32) < 1:
        fail('--max-skipped-steps must be at least 1')
    oib = getattr(args, 'optimizer_in_backward', 'auto')
    if oib == 'on':
        fail('--optimizer-in-backward on cannot be combined with --clip-grad-norm / '
             '--skip-nonfinite-steps: a bucket updated during the backward cannot wait '
             'for the global gradient norm of the step')
    if oib == 'auto':
        args.optimizer_in_backward = 'off'
    return args


def validate_train_args(args):             # utils/options.py:318-325
    args = validate_dataset_args(args)
    assert args.bs > 0
    assert args.mbs > 0
    assert args.bs % args.mbs == 0
    args.accum_step = args.bs // args.mbs
    assert args.permanent_interval % args.checkpointing_interval == 0
    if getattr(args, 'representation_deterministic', False) and \
            not getattr(args, 'learnable_representation', False):
        raise SystemExit('--representation-deterministic needs --learnable-representation')
    return validate_compact_event_terms_args(validate_capture_event_terms_args(validate_frameless_args(
        validate_sharpness_args(validate_avg_timestamp_args(validate_contrast_args(args))))))


def validate_compact_event_terms_args(args):
    """--compact-event-terms (absent from ``args`` unless given) against what
    it needs: --compact-events, and a term to read those columns.  With it the
    two terms do not refuse --compact-events (validate_contrast_args,
    validate_avg_timestamp_args)."""
    if not getattr(args, 'compact_event_terms', False):
        return args
    if not getattr(args, 'compact_events', False):
        raise SystemExit('--compact-event-terms needs --compact-events: it says what reads the '
                         'encoded event columns')
    if not (getattr(args, 'contrast_weight', 0.0) > 0 or getattr(args, 'avg_timestamp_weight', 0.0) > 0):
        raise SystemExit('--compact-event-terms needs a positive --contrast-weight or '
                         '--avg-timestamp-weight: without either there is no events-only term to '
                         'feed')
    return args


def validate_capture_event_terms_args(args):
    """--capture-event-terms (absent from ``args`` unless given) against what
    it needs: --capture, and a term to carry."""
    if not getattr(args, 'capture_event_terms', False):
        return args
    if not getattr(args, 'capture', False):
        raise SystemExit('--capture-event-terms needs --capture: it says what the captured step '
                         'carries')
    if not (getattr(args, 'contrast_weight', 0.0) > 0 or getattr(args, 'avg_timestamp_weight', 0.0) > 0):
        raise SystemExit('--capture-event-terms needs a positive --contrast-weight or '
                         '--avg-timestamp-weight: without either there is no events-only term to '
                         'capture')
    return args


CONTRAST_REFERENCE_NAMES = ('start', 'middle', 'end')


def parse_contrast_references(text, option='--contrast-references'):
    """'end,start' -> ('start', 'end'): the names in the order of the window."""
    names = [n.strip() for n in text.split(',')] if isinstance(text, str) else list(text)
    for n in names:
        if n not in CONTRAST_REFERENCE_NAMES:
            raise SystemExit(f'{option}: unknown reference time "{n}", '
                             f'one of {", ".join(CONTRAST_REFERENCE_NAMES)}')
        if names.count(n) > 1:
            raise SystemExit(f'{option}: "{n}" is given twice')
    return tuple(n for n in CONTRAST_REFERENCE_NAMES if n in names)


def validate_contrast_args(args):
    """--contrast-weight against what it cannot be combined with, and the
    term's options against a run without the term.  ``args.contrast_references``
    becomes a tuple of names."""
    weight = getattr(args, 'contrast_weight', 0.0)
    if weight < 0 or weight != weight:
        raise SystemExit(f'--contrast-weight must not be negative, got {weight}')
    args.contrast_references = parse_contrast_references(getattr(args, 'contrast_references', 'start'))
    args.contrast_polarity = bool(getattr(args, 'contrast_polarity', False))
    if not weight > 0:
        if args.contrast_references != ('start',):
            raise SystemExit('--contrast-references needs a positive --contrast-weight')
        if args.contrast_polarity:
            raise SystemExit('--contrast-polarity needs a positive --contrast-weight')
        if getattr(args, 'contrast_scales', 'finest') != 'finest':     # absent unless given
            raise SystemExit('--contrast-scales needs a positive --contrast-weight')
    if weight > 0 and getattr(args, 'ev_images', False):
        raise SystemExit('--contrast-weight cannot be combined with --ev_images: the term is '
                         'computed from the raw events on the device, and a batch of '
                         'preprocessed event images carries none')
    if weight > 0 and getattr(args, 'compact_events', False) and not getattr(args, 'compact_event_terms', False):
        raise SystemExit('--contrast-weight cannot be combined with --compact-events: the term '
                         'reads the int64 / float32 wire columns, not the 9 B/event encoded ones')
    return args


AVG_TIMESTAMP_REFERENCES = ('start', 'end')


def validate_avg_timestamp_args(args):
    """--avg-timestamp-weight against what it cannot be combined with, and the
    term's options against a run without the term.  The options are
    absent from ``args`` unless given (read them with ``getattr``); a given
    ``args.avg_timestamp_references`` becomes a tuple of names."""
    weight = getattr(args, 'avg_timestamp_weight', 0.0)
    if weight < 0 or weight != weight:
        raise SystemExit(f'--avg-timestamp-weight must not be negative, got {weight}')
    if hasattr(args, 'avg_timestamp_references'):
        args.avg_timestamp_references = parse_contrast_references(args.avg_timestamp_references,
                                                                  '--avg-timestamp-references')
    if not weight > 0:
        if hasattr(args, 'avg_timestamp_references'):
            raise SystemExit('--avg-timestamp-references needs a positive --avg-timestamp-weight')
        if getattr(args, 'avg_timestamp_polarity', False):
            raise SystemExit('--avg-timestamp-polarity needs a positive --avg-timestamp-weight')
        if getattr(args, 'avg_timestamp_scales', 'finest') != 'finest':     # absent unless given
            raise SystemExit('--avg-timestamp-scales needs a positive --avg-timestamp-weight')
    if weight > 0 and getattr(args, 'ev_images', False):
        raise SystemExit('--avg-timestamp-weight cannot be combined with --ev_images: the term is '
                         'computed from the raw events on the device, and a batch of '
                         'preprocessed event images carries none')
    if weight > 0 and getattr(args, 'compact_events', False) and not getattr(args, 'compact_event_terms', False):
        raise SystemExit('--avg-timestamp-weight cannot be combined with --compact-events: the term '
                         'reads the int64 / float32 wire columns, not the 9 B/event encoded ones')
    return args


def avg_timestamp_keywords(args):
    """The keywords of training.train / validate / hooks.ValidationHook for
    the average-timestamp term: none unless --avg-timestamp-weight is positive."""
    weight = getattr(args, 'avg_timestamp_weight', 0.0)
    if not weight:
        return {}
    out = {'avg_timestamp_weight': weight,
           'avg_timestamp_references': tuple(getattr(args, 'avg_timestamp_references', AVG_TIMESTAMP_REFERENCES)),
           'avg_timestamp_polarity': bool(getattr(args, 'avg_timestamp_polarity', False))}
    if getattr(args, 'avg_timestamp_scales', 'finest') != 'finest':     # only where it differs from the default
        out['avg_timestamp_scales'] = args.avg_timestamp_scales
    return out


def validate_sharpness_args(args):
    """The options of the sharpness measurement against a run without it.
    ``args.sharpness_references`` becomes a tuple of names."""
    args.sharpness_references = parse_contrast_references(getattr(args, 'sharpness_references', 'start'),
                                                          '--sharpness-references')
    args.sharpness_polarity = bool(getattr(args, 'sharpness_polarity', False))
    if not getattr(args, 'sharpness_period', 0) > 0:
        if args.sharpness_references != ('start',):
            raise SystemExit('--sharpness-references needs a positive --sharpness-period')
        if args.sharpness_polarity:
            raise SystemExit('--sharpness-polarity needs a positive --sharpness-period')
        if getattr(args, 'sharpness_rsat', False):
            raise SystemExit('--sharpness-rsat needs a positive --sharpness-period')
    return args


def validate_frameless_args(args):
    """--recording / --validation-recording (docs/FRAMELESS_SPEC.md) against
    what they need and what they cannot be combined with.  Without them
    nothing is looked at but the two window flags, which need one of them."""
    recording = getattr(args, 'recording', None)
    validation = getattr(args, 'validation_recording', None)
    duration = getattr(args, 'window_duration', None)
    events = getattr(args, 'window_events', None)
    if recording is None and validation is None:
        for flag, value in (('--window-duration', duration), ('--window-events', events)):
            if value is not None:
                raise SystemExit(f'{flag} needs --recording or --validation-recording')
        return args
    which = '--recording' if recording is not None else '--validation-recording'
    if (duration is None) == (events is None):
        raise SystemExit(f'{which} needs exactly one of --window-duration and --window-events')
    if duration is not None and not (duration > 0 and duration != float('inf')):
        raise SystemExit(f'--window-duration must be positive and finite, got {duration}')
    if events is not None and events < 1:
        raise SystemExit(f'--window-events must be at least 1, got {events}')
    weight = getattr(args, 'contrast_weight', 0.0)
    if recording is not None:
        if not weight > 0:
            raise SystemExit('--recording needs --contrast-weight > 0: without frames the '
                             'contrast-maximisation term is the only data term')
        for flag, value in (('--sequence', getattr(args, 'sequence', None) is not None),
                            ('--synthetic', getattr(args, 'synthetic', False)),
                            ('--preprocessed-dataset-path',
                             getattr(args, 'preprocessed_dataset_path', None) is not None),
                            ('--ev_images', getattr(args, 'ev_images', False)),
                            ('--compact-events', getattr(args, 'compact_events', False)),
                            ('--device-feeder', getattr(args, 'device_feeder', False))):
            if value:
                raise SystemExit(f'--recording cannot be combined with {flag}: the batches are '
                                 'cut from the event-only recording on the device')
    if validation is not None:
        if getattr(args, 'validation_sequence', None) is not None:
            raise SystemExit('--validation-recording cannot be combined with '
                             '--validation-sequence: one validation source')
        if not weight > 0 and not getattr(args, 'skip_validation', False):
            raise SystemExit('--validation-recording needs --contrast-weight > 0 (or '
                             '--skip-validation): a frameless validation loss has no other '
                             'data term')
        if getattr(args, 'visualization_period', 0) > 0:
            raise SystemExit('--visualization-period cannot be combined with '
                             '--validation-recording: its pictures show grey images, and a '
                             'frameless recording has none')
        if getattr(args, 'evaluation_period', 0) > 0:
            raise SystemExit('--evaluation-period cannot be combined with '
                             '--validation-recording: the evaluation hook needs '
                             '--validation-sequence (grey images under its pictures)')
    return args


def window_kwargs(args):
    """The window arguments of ``sequence.WindowedEvents.from_file``."""
    if getattr(args, 'window_duration', None) is not None:
        return {'duration': args.window_duration}
    return {'events_per_window': args.window_events}


def options2dataset_kwargs(parameters):    # utils/options.py:332-338
    return dict(prefix_length=parameters.prefix_length,
                suffix_length=parameters.suffix_length,
                max_sequence_length=parameters.max_sequence_length,
                dynamic_sample_length=parameters.dynamic_sample_length,
                event_representation_depth=parameters.
                event_representation_depth)


def options2model_kwargs(parameters):      # utils/options.py:341-347
    kwargs = options2dataset_kwargs(parameters)
    kwargs['activation'] = Mish() if parameters.mish else nn.ReLU()
    # MI355X build only; models without this ctor argument never see it
    # (model.init_model filters by signature, utils/model.py:10-23)
    if getattr(parameters, 'compute_dtype', 'f32') != 'f32':
        kwargs['compute_dtype'] = parameters.compute_dtype
    if getattr(parameters, 'learnable_representation', False):
        kwargs['learnable_representation'] = True
        kwargs['representation_radius'] = parameters.representation_radius
        kwargs['representation_knots'] = parameters.representation_knots
        if getattr(parameters, 'representation_resident', False):
            kwargs['representation_resident'] = True
        if getattr(parameters, 'representation_deterministic', False):
            kwargs['representation_deterministic'] = True
    return kwargs

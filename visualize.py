#!/usr/bin/env python3
"""The reference's visualize.py (:24-207) on this package: every sample of
the validation data, one at a time (``mbs = 1``), as ``NNNN.png`` (frames on
top, the predicted flow pyramid below; docs/RENDER_SPEC.md) and ``NNNN.yml``
(loss terms, event counts, each level's colour scale) under
``visualization/<model name>/<name of --sp, or step_0>/`` of the working
directory.  Samples whose two files exist are skipped.  Takes the training
flags; the weights are those of ``--sp``.  The pictures are drawn on the
device; a writer thread compresses and writes them (the reference: a process
pool around the host rendering)."""
import queue
import sys
import threading
from pathlib import Path

import torch
import yaml

import train_flownet as tf
from dvs_of_training_framework_amd.loss import init_losses
from dvs_of_training_framework_amd.model import init_model
from dvs_of_training_framework_amd.timer import FakeTimer
from dvs_of_training_framework_amd.training import process_minibatch
from dvs_of_training_framework_amd.visualization import visualize, write_png


def choose_output_path(args):              # visualize.py:143-153
    step = 'step_0' if args.sp is None else Path(args.sp).stem
    path = Path('visualization') / args.model.name / step
    path.mkdir(parents=True, exist_ok=True)
    return path


def files(filename):                       # visualize.py:170-173
    return filename.parent / (filename.name + '.png'), \
        filename.parent / (filename.name + '.yml')


def image_writer(image_queue, errors):     # visualize.py:156-167
    while True:
        data = image_queue.get()
        if data is None:
            return
        try:
            path, image, statistics = data
            image_file, yaml_file = files(path)
            if not image_file.is_file():
                write_png(image_file, image)
            if not yaml_file.is_file():
                with yaml_file.open('w') as f:
                    yaml.dump(statistics, f)
        except Exception as e:              # surfaces on the main thread
            errors.append(e)


def main(argv=None):
    """-> the number of samples written."""
    args = tf.parse_args(sys.argv[1:] if argv is None else argv)
    args.mbs = 1
    device = torch.device(args.device)
    output_dir = choose_output_path(args)
    model = init_model(args, device)
    model.eval()
    loader = tf.make_validation_loader(args, device)
    if loader is None:
        raise SystemExit('no validation data (--validation-sequence, or '
                         '--synthetic-validation-batches with --synthetic)')
    evaluator = init_losses(args.shape, 1, model, device,
                            sequence_length=args.prefix_length + args.suffix_length + 1)
    image_queue, errors, written = queue.Queue(maxsize=8), [], 0
    writer = threading.Thread(target=image_writer, args=(image_queue, errors))
    writer.start()
    try:
        with torch.no_grad():
            for i, batch in enumerate(loader):
                output_file_path = output_dir / f'{i:04d}'
                if all(x.is_file() for x in files(output_file_path)):
                    continue
                loss, parts, tags, prediction = process_minibatch(
                    model, batch, FakeTimer(), device, args.is_raw, evaluator,
                    args.loss_weights, return_prediction=True)
                image, statistics = visualize(args, batch, loss, parts,
                                              args.loss_weights, prediction)
                image_queue.put((output_file_path, image, statistics))
                written += 1
    finally:
        image_queue.put(None)
        writer.join()
    if errors:
        raise errors[0]
    return written


if __name__ == '__main__':
    main()

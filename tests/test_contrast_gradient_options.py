"""What ``Losses.contrast(objective=)``, ``Losses.event_terms`` and
``--contrast-objective`` refuse, each naming its condition; ``variance`` is taken everywhere."""
import pytest
import torch

import train_flownet as tf
from dvs_of_training_framework_amd import loss as L

GRADIENT = ['--contrast-weight', '0.25', '--contrast-objective', 'gradient']


@pytest.mark.parametrize('extra,refusal', [
    (GRADIENT, None),
    (GRADIENT + ['--contrast-references', 'start,middle,end', '--contrast-polarity', '--capture'], None),
    (['--contrast-weight', '0.25', '--contrast-objective', 'variance', '--contrast-scales', 'all'], None),
    (['--contrast-objective', 'variance'], None),
    (['--contrast-objective', 'gradient'], 'needs a positive --contrast-weight'),
    (GRADIENT + ['--contrast-scales', 'all'], '--contrast-scales all'),
    (GRADIENT + ['--event-images-tiled'], '--event-images-tiled'),
    (GRADIENT + ['--avg-timestamp-weight', '0.5', '--avg-timestamp-scales', 'all', '--event-pyramids-tiled'],
     '--event-pyramids-tiled'),
    (GRADIENT + ['--avg-timestamp-weight', '0.5', '--event-terms-joint'], '--event-terms-joint'),
    (GRADIENT + ['--capture', '--capture-event-terms'], '--capture-event-terms')])
def test_the_parser_takes_the_objective_where_it_has_a_form(extra, refusal, tmp_path):
    model = ['-m', str(tmp_path / 'm'), '--synthetic']
    if refusal is None:
        assert getattr(tf.parse_args(model + extra), 'contrast_objective') == extra[extra.index(
            '--contrast-objective') + 1]
    else:
        with pytest.raises(SystemExit, match='--contrast-objective gradient.*' + refusal):
            tf.parse_args(model + extra)
    assert not hasattr(tf.parse_args(model), 'contrast_objective')      # the run without the flag


@pytest.mark.parametrize('kw,refusal', [
    (dict(objective='gradient', scales='all'), 'finest scale'), (dict(objective='gradient', tiled=True), 'tiled=True'),
    (dict(objective='gradient', tiled='force'), 'tiled=.force'),
    (dict(objective='sharpness'), 'unknown contrast objective')])
def test_losses_contrast_refuses_before_it_looks_at_anything(kw, refusal):
    losses = L.Losses([(4, 4)], 1, 'cpu')
    with pytest.raises(ValueError, match=refusal):
        losses.contrast([torch.zeros(1, 2, 4, 4)], None, None, {}, **kw)
    with pytest.raises(ValueError, match='objective "gradient" has no joint call'):
        losses.event_terms([torch.zeros(1, 2, 4, 4)], None, None, {}, dict(weight=0.25, objective='gradient'),
                           dict(weight=0.5))

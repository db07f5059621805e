"""What the census term refuses on the host, each naming its condition, and
that weight 0 asks the evaluator for nothing (docs/CENSUS_SPEC.md)."""
import pytest
import torch

import train_flownet as tf
from dvs_of_training_framework_amd import training


class _Evaluator:
    def __call__(self, flows, *rest, **kw):
        return tuple(tuple(torch.tensor(float(10 * t + k)) for k in range(len(flows))) for t in range(3))

    def census(self, flows, flow_ts, flow_sample_idx, images, timestamps, sample_idx, weight=None, **kw):
        terms = torch.tensor([2.0, 4.0])
        return weight * terms.mean(), terms

    def frameless(self, flows, weights):
        return torch.tensor(1.0), torch.zeros(3, len(flows))


def test_combined_loss_carries_the_term_and_refuses_by_name():
    flows = (torch.zeros(1, 2, 2, 2), torch.zeros(1, 2, 4, 4))
    call = (_Evaluator(), flows, None, None, torch.zeros(2, 4, 4), None, None, None)
    plain, terms = training.combined_loss(*call)
    same, terms_ = training.combined_loss(*call, census_weight=0.0)
    assert float(same) == float(plain) and type(terms_) is type(terms) is tuple
    loss, carried = training.combined_loss(*call, census_weight=0.25)
    assert float(loss) == float(plain) + 0.75 and carried.census.tolist() == [2.0, 4.0]
    assert carried.contrast is None and carried.avg_timestamp is None and len(carried) == 3
    back = training.TermReadback(carried)
    assert back.census() == 3.0 and back.census_levels() == [2.0, 4.0] and back.contrast() is None
    assert training.TermReadback(terms).census() is None
    with pytest.raises(ValueError, match='census_weight must not be negative, got -0.5'):
        training.combined_loss(*call, census_weight=-0.5)
    frameless = call[:4] + (None,) + call[5:]
    with pytest.raises(ValueError, match='census_weight > 0 needs frames'):
        training.combined_loss(*frameless, census_weight=0.25, contrast_weight=0.25, events={'x': None})


def test_the_capture_refusal_names_the_flag():
    assert training.census_capture_refusal() is None and training.census_capture_refusal(0.0) is None
    assert '--census-weight 0.25' in training.census_capture_refusal(0.25)
    assert 'dvsof_census_fwd' in training.census_capture_refusal(0.25)


@pytest.mark.parametrize('extra,refusal', [
    (['--census-weight', '0.25'], None),
    (['--census-weight', '0.25', '--contrast-weight', '0.5', '--avg-timestamp-weight', '0.5', '--capture'], None),
    (['--census-weight', '-1'], 'must not be negative'),
    (['--census-weight', '0.25', '--contrast-weight', '0.5', '--recording', 'r.npz', '--window-events', '100'],
     '--census-weight 0.25 cannot be combined with --recording'),
    (['--census-weight', '0.25', '--validation-recording', 'r.npz', '--window-events', '100'],
     '--census-weight 0.25 cannot be combined with --validation-recording')])
def test_the_parser_refuses_the_term_without_frames(extra, refusal, tmp_path):
    model = ['-m', str(tmp_path / 'm'), '--synthetic']
    if refusal is None:
        assert tf.parse_args(model + extra).census_weight == 0.25
    else:
        with pytest.raises(SystemExit, match=refusal):
            tf.parse_args(model + extra)
    assert not hasattr(tf.parse_args(model), 'census_weight')       # the run without the flag

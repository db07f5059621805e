"""serializer.Serializer on the CPU (the plain path): the reference's rules
for permanent / temporal checkpoints and pruning (utils/serializer.py:37-148),
restated as hand-written expectations; atomic files; refusal of non-finite
state; the writer thread's error protocol; files that hold each tensor's own
bytes only."""
import math
import os

import pytest
import torch

from dvs_of_training_framework_amd.serializer import (
    Serializer, count_nonfinite, own_storage, template_regex)


def make(seed=0, steps=1):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 2))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2, amsgrad=True)
    for _ in range(steps):
        opt.zero_grad()
        model(torch.ones(3, 5)).sum().backward()
        opt.step()
    return model, opt


def names(path):
    return sorted(p.name for p in path.iterdir())


# --------------------------------------------------------------- the rules
@pytest.mark.parametrize('interval,permanent', [
    (0, []),                        # 0: no permanent checkpoints at all
    (1, list(range(10))),           # 1: every step is permanent
    (4, [0, 4, 8]),                 # step 0 is permanent whenever the interval is > 0
])
def test_permanent_and_temporal_sets(tmp_path, interval, permanent):
    model, opt = make()
    s = Serializer(tmp_path, keep_checkpoints_max=2,
                   permanent_checkpoint_interval=interval)
    for step in range(10):
        s.checkpoint_model(model, opt, step)
    temporal = [k for k in range(10) if k not in permanent][-2:]   # the newest two
    assert s.list_known_steps() == sorted(permanent + temporal)
    assert names(tmp_path) == sorted(f'step_{k}.pt' for k in permanent + temporal)
    assert s.has_checkpoints()


def test_pruning_order_is_by_step_not_by_time(tmp_path):
    model, opt = make()
    s = Serializer(tmp_path, keep_checkpoints_max=2, permanent_checkpoint_interval=0)
    for step in (7, 3, 9, 5):       # written out of order: the two largest stay
        s.checkpoint_model(model, opt, step)
    assert s.list_known_steps() == [7, 9]


@pytest.mark.parametrize('keep', [0, -1, math.inf])
def test_keep_all(tmp_path, keep):
    model, opt = make()
    s = Serializer(tmp_path, keep_checkpoints_max=keep, permanent_checkpoint_interval=0)
    for step in range(5):
        s.checkpoint_model(model, opt, step)
    assert s.list_known_steps() == [0, 1, 2, 3, 4]


def test_found_on_disk_foreign_names_ignored_stale_tmp_removed(tmp_path):
    model, opt = make()
    s = Serializer(tmp_path, 3, 4)
    for step in (0, 1, 2, 4):
        s.checkpoint_model(model, opt, step)
    for foreign in ('step_x.pt', 'step_3.pth', 'xstep_3.pt', 'step_-1.pt', 'step_3.pt.bak',
                    'notes.tmp'):
        (tmp_path / foreign).write_bytes(b'?')
    (tmp_path / 'log').mkdir()
    (tmp_path / 'step_9.pt.tmp').write_bytes(b'half a checkpoint')
    again = Serializer(tmp_path, 3, 4)
    assert again.list_known_steps() == [0, 1, 2, 4]
    assert not (tmp_path / 'step_9.pt.tmp').exists()
    assert (tmp_path / 'notes.tmp').exists()            # not this serializer's
    assert sorted(again._permanent_checkpoints) == [0, 4]
    assert sorted(again._temporal_checkpoints) == [1, 2]
    assert not Serializer(tmp_path / 'empty').has_checkpoints()


def test_template():
    assert template_regex('step_{}.pt').fullmatch('step_12.pt').group(1) == '12'
    assert template_regex('m.{}').fullmatch('mx3') is None      # '.' is literal
    for bad in ('step.pt', 'step_{}_{}.pt'):
        with pytest.raises(ValueError):
            template_regex(bad)


def test_schema_load_and_finalize(tmp_path):
    model, opt = make(steps=2)
    s = Serializer(tmp_path)
    rng_state = {'bit_generator': 'PCG64', 'state': {'state': 2 ** 127 + 5, 'inc': 2 ** 100 + 1},
                 'has_uint32': 0, 'uinteger': 0}
    s.checkpoint_model(model, opt, 6, samples_passed=24,
                       loader_state=[{'rng': rng_state, 'drawn': 3}])
    file = torch.load(tmp_path / 'step_6.pt', weights_only=True)
    assert set(file) == {'model', 'optimizer', 'global_step', 'samples_passed', 'loader_state'}
    assert file['global_step'] == 6 and file['loader_state'][0]['rng'] == rng_state
    other, other_opt = make(seed=1)
    step, rest = s.load_checkpoint(other, 6, optimizer=other_opt)
    assert step == 6 and set(rest) == {'samples_passed', 'loader_state'}
    for a, b in zip(model.state_dict().values(), other.state_dict().values()):
        assert torch.equal(a, b)
    want, got = opt.state_dict(), other_opt.state_dict()
    assert got['param_groups'] == want['param_groups']
    for k, st in want['state'].items():
        for name, v in st.items():
            assert torch.equal(got['state'][k][name], v)
    with pytest.raises(ValueError, match='step 5 not found'):
        s.load_checkpoint(other, 5)
    s.finalize(6, tmp_path / 'final.pt')
    bare = torch.load(tmp_path / 'final.pt', weights_only=True)
    assert list(bare) == list(model.state_dict())
    assert all(torch.equal(bare[k], v) for k, v in model.state_dict().items())


# --------------------------------------------------------------- atomicity
def test_a_failed_rename_leaves_the_previous_checkpoint(tmp_path):
    model, opt = make()
    s = Serializer(tmp_path, keep_checkpoints_max=1, permanent_checkpoint_interval=0)
    s.checkpoint_model(model, opt, 1)

    def broken(src, dst):
        raise OSError('disk went away')
    s._replace = broken
    with pytest.raises(OSError, match='disk went away'):        # the plain path: this call
        s.checkpoint_model(model, opt, 2)
    assert s.list_known_steps() == [1]                          # neither listed nor pruned for
    assert names(tmp_path) == ['step_1.pt', 'step_2.pt.tmp']
    assert s.load_checkpoint(model, 1)[0] == 1
    s._replace = os.replace
    s.checkpoint_model(model, opt, 3)
    assert names(tmp_path) == ['step_2.pt.tmp', 'step_3.pt']
    assert Serializer(tmp_path, 1, 0).list_known_steps() == [3]
    assert names(tmp_path) == ['step_3.pt']


def test_an_error_of_the_writer_thread_is_raised_by_the_next_call(tmp_path):
    model, opt = make()
    s = Serializer(tmp_path, 1, 0)
    s.checkpoint_model(model, opt, 1)
    state = {'model': model.state_dict(), 'optimizer': opt.state_dict(), 'global_step': 2}

    def broken(src, dst):
        raise OSError('disk went away')
    s._replace = broken
    s._enqueue(lambda: s._commit(state, 2))     # what the asynchronous path hands its thread
    with pytest.raises(RuntimeError, match='disk went away'):
        s.checkpoint_model(model, opt, 3)       # the NEXT call surfaces it
    assert s.list_known_steps() == [1] and s.load_checkpoint(model, 1)[0] == 1
    s._replace = os.replace
    s._enqueue(lambda: s._commit(dict(state), 2))
    s.wait()                                    # raised once, not again
    assert s.list_known_steps() == [2]
    s._replace = broken
    s._enqueue(lambda: s._commit(dict(state), 4))
    with pytest.raises(RuntimeError, match='disk went away'):
        s.wait()
    s._enqueue(lambda: s._commit(dict(state), 4))
    with pytest.raises(RuntimeError, match='disk went away'):
        s.close()
    assert s._thread is None


# ----------------------------------------------------------------- refusal
@pytest.mark.parametrize('where', ['parameter', 'exp_avg_sq'])
def test_non_finite_state_is_refused(tmp_path, capsys, where):
    model, opt = make()
    s = Serializer(tmp_path, keep_checkpoints_max=2, permanent_checkpoint_interval=0)
    s.checkpoint_model(model, opt, 1)
    s.checkpoint_model(model, opt, 2)
    with torch.no_grad():
        if where == 'parameter':
            model[0].weight[1, 2] = float('nan')
            model[1].bias[0] = float('nan')
            planted = 2
        else:
            opt.state[model[1].weight]['exp_avg_sq'][0, 0] = float('inf')
            planted = 1
    before = names(tmp_path)
    assert s.checkpoint_model(model, opt, 3) is False
    assert s.checkpoint_model(model, opt, 4) is False
    assert names(tmp_path) == before == ['step_1.pt', 'step_2.pt']     # two bad ones pruned nothing
    assert s.refused == [(3, planted), (4, planted)]
    err = capsys.readouterr().err
    assert 'step 3' in err and f'{planted} non-finite' in err
    assert not err.startswith('capture:') and 'could not be recorded' not in err


def test_count_nonfinite_counts_a_shared_tensor_once():
    t = torch.tensor([1.0, float('nan'), float('-inf')])
    assert count_nonfinite({'a': t, 'b': [t, torch.tensor([float('inf')])], 'n': 3}) == 3
    assert count_nonfinite({'i': torch.tensor([1, 2])}) == 0


# ------------------------------------------------------------- file size
def test_saved_tensors_own_their_storage(tmp_path):
    """A parameter that is a 10-element view of a 1 M-element buffer is saved
    as 40 bytes, not as 4 MB; two entries that are one tensor stay one."""
    big = torch.zeros(1 << 20)
    model = torch.nn.Linear(5, 2)
    model.weight = torch.nn.Parameter(big[7:17].view(2, 5))
    model.bias = torch.nn.Parameter(big[100:102])
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    model(torch.ones(1, 5)).sum().backward()
    opt.step()
    s = Serializer(tmp_path)
    s.checkpoint_model(model, opt, 1)
    tensor_bytes = 4 * (10 + 2) * 2         # parameters and momentum buffers
    assert (tmp_path / 'step_1.pt').stat().st_size < tensor_bytes + 8192   # zip + pickle overhead
    file = torch.load(tmp_path / 'step_1.pt', weights_only=True)
    assert torch.equal(file['model']['weight'], model.weight)
    view = big[:6].view(2, 3).t()           # strides survive
    shared = own_storage({'a': view, 'b': view, 'c': big[:6]})
    assert shared['a'] is shared['b'] and shared['a'].stride() == (1, 3)
    assert shared['a'].untyped_storage().nbytes() <= 4 * 6
    assert shared['c'].data_ptr() != shared['a'].data_ptr()

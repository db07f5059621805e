"""World-size-2 checkpoint hook on CPU (gloo, the plain path): every rank runs
the hook, rank 0 alone writes ONE file holding both ranks' loader states; on
resume each rank takes its own entry, and a one-process run refuses the file."""
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Loader:
    def __init__(self, at):
        self.at = at

    def state(self):
        return {'next': self.at}

    def restore(self, state):
        self.at = state['next']


def _worker(rank, world, port, path, q):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    import train_flownet as tf
    from dvs_of_training_framework_amd import parallel
    from dvs_of_training_framework_amd.hooks import SerializationHook
    from dvs_of_training_framework_amd.serializer import Serializer
    parallel.init_distributed('cpu')
    torch.manual_seed(0)
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    model(torch.ones(1, 3)).sum().backward()
    opt.step()
    serializer = Serializer(path, async_snapshot=False)
    loader = _Loader(100 + 7 * rank)
    hook = SerializationHook(
        serializer, model, opt, None,
        lambda: {'world_size': world, 'loader_state': loader.state()}, rank=rank)
    hook(4, 32)
    dist.barrier()
    files = sorted(p.name for p in Path(path).iterdir())
    # resume: every rank reads the one file and takes its own entry
    again = Serializer(path, async_snapshot=False)
    step, state = again.load_checkpoint(model, again.list_known_steps()[-1], optimizer=opt)
    tf.check_resume_world(state, world, 'the file')
    mine = _Loader(0)
    tf.restore_loader(mine, state, rank, world, step, None)
    q.put((rank, files, step, state['samples_passed'], state['world_size'],
           len(state['loader_state']), mine.at))
    dist.destroy_process_group()


def test_one_file_two_loader_states(tmp_path):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, files, step, samples, world, n_states, at in res:
        assert files == ['step_4.pt']
        assert (step, samples, world, n_states) == (4, 32, 2, 2)
        assert at == 100 + 7 * rank
    # one process refuses to continue it
    import train_flownet as tf
    state = torch.load(tmp_path / 'step_4.pt', weights_only=True)
    assert [s['next'] for s in state['loader_state']] == [100, 107]
    with pytest.raises(SystemExit, match='written by 2 process.*--do_not_continue'):
        tf.check_resume_world(state, 1, tmp_path / 'step_4.pt')
    tf.check_resume_world({'samples_passed': 3}, 1, 'a reference checkpoint')   # no entry: one process

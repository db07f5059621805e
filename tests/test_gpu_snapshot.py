"""The checkpoint snapshot on the GPU: the gather kernel bit for bit against
the flattened storages (every size class, alignment, layout, special value,
the untouched gaps, the non-finite count), and the asynchronous checkpoint of
the three fused optimizers against ``state_dict()`` at the same step."""
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 0x5A5A5A5A          # a finite float: a gap that was counted would show
PAST = 1024                    # floats behind the slab's end that must stay as they are


def storage_order(t):
    """The numel floats of a dense tensor as they lie in memory, as int32."""
    return torch.as_strided(t, (t.numel(),), (1,)).view(torch.int32)


@pytest.fixture(scope='module')
def packed():
    """Two launches into one slab, shared by the tests below: a healthy state
    (parity 0), then the same tensors with NaN / Inf planted (parity 1)."""
    from dvs_of_training_framework_amd import _lib, snapshot
    chunk = _lib.lib().dvsof_snapshot_chunk_elems()
    sizes = [1, 3, 4, 5, 1023, 1024, 1025, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]
    g = torch.Generator(device='cpu').manual_seed(11)
    tensors, names = [], []
    for n in sizes:
        for a in range(4):      # source 0, 4, 8, 12 bytes past a 16-byte aligned address
            buf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
            assert buf.data_ptr() % 16 == 0
            src = buf[a:a + n]
            src.copy_(torch.randn(n, generator=g))
            tensors.append(src)
            names.append((n, a))
    empty = torch.empty(0, dtype=torch.float32, device=DEV)
    weight = torch.randn(6, 5, 3, 3, generator=g).to(DEV).contiguous(
        memory_format=torch.channels_last)
    assert weight.stride() == (45, 1, 15, 5)
    special = torch.tensor([0x80000000, 0x00000001, 0x807fffff, 0x00400000, 0x3f800000],
                           dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV)
    tensors += [empty, weight, special, weight]      # the weight is listed twice
    names += ['empty', 'weight', 'special', 'weight again']

    entries, index, total = snapshot.slab_layout(tensors)
    slab = torch.full((total + PAST,), SENTINEL, dtype=torch.int32, device=DEV)
    slab[0] = 0                 # the first launch adds into a word nobody zeroed for it
    snapshot.pack(tensors, slab, parity=0)
    torch.cuda.synchronize()
    healthy = slab.cpu()
    want_healthy = expected(entries, total, parity=0, count=0)
    flat_healthy = torch.cat([storage_order(t).cpu() for t, _ in entries])

    # plant: {(tensor name): [(element, bits)]}
    plant = {
        (1025, 0): [(0, 0x7fc12345)],                       # first element, quiet NaN payload
        (1023, 2): [(1022, 0xff800000)],                    # last element, -Inf
        (2 * chunk + 7, 0): [(chunk - 1, 0x7f800000), (chunk, 0x7f800001),      # chunk boundary
                             (2 * chunk + 6, 0xffc00001)],  # and the scalar tail of the last chunk
        (5, 0): [(4, 0x7f800000)],                          # scalar tail (float4 path)
        (3, 2): [(2, 0x7fffffff)],                          # scalar tail (float2 path)
        (chunk + 1, 1): [(chunk, 0x7f812345)],              # 4-byte aligned source
        (1024, 3): [(17, 0xff800000)],
        'weight': [(269, 0x7fc00000)],                      # listed twice, counted once
    }
    planted = 0
    for name, spots in plant.items():
        t = tensors[names.index(name)]
        flat = storage_order(t)
        for element, bits in spots:
            flat[element] = bits - (1 << 32) if bits >= (1 << 31) else bits
            planted += 1
    snapshot.pack(tensors, slab, parity=1)
    torch.cuda.synchronize()
    return dict(chunk=chunk, tensors=tensors, names=names, entries=entries, index=index,
                total=total, healthy=healthy, want_healthy=want_healthy,
                flat_healthy=flat_healthy, poisoned=slab.cpu(),
                want_poisoned=expected(entries, total, parity=1, count=planted),
                planted=planted)


def expected(entries, total, parity, count):
    """The slab as the specification says it must look: header, every entry's
    storage at its offset (``torch.cat`` of the flattened storages where the
    entries touch), the sentinel everywhere else."""
    want = torch.full((total + PAST,), SENTINEL, dtype=torch.int32)
    want[parity], want[parity ^ 1] = count, 0
    for t, off in entries:
        want[off:off + t.numel()] = storage_order(t).cpu()
    return want


def test_layout(packed):
    from dvs_of_training_framework_amd import snapshot
    offs = [off for _, off in packed['entries']]
    assert offs[0] == snapshot.HEADER_FLOATS == 4
    assert all(off % 4 == 0 for off in offs)                # 16-byte destinations
    for (t, off), nxt in zip(packed['entries'], offs[1:] + [packed['total']]):
        assert 0 <= nxt - off - t.numel() < 4               # dense: gaps are padding only
    assert packed['index'][-1] == packed['index'][-3]       # one entry for the weight
    assert len(packed['entries']) == len(packed['tensors']) - 1


def test_healthy_state_bit_for_bit(packed):
    got, want = packed['healthy'], packed['want_healthy']
    assert got[0] == 0 and got[1] == 0, 'count of a healthy state, next header word zeroed'
    assert got[2] == SENTINEL and got[3] == SENTINEL
    assert torch.equal(got, want)       # data, alignment gaps and everything past the end
    # the same, said with torch.cat of the flattened storages
    pieces = packed['flat_healthy']      # (taken before the second launch's values were planted)
    where = torch.cat([torch.arange(off, off + t.numel()) for t, off in packed['entries']])
    assert torch.equal(got[where], pieces)


def test_special_values_and_layout_survive(packed):
    e = packed['index'][packed['names'].index('special')]
    off = packed['entries'][e][1]
    got = packed['healthy'][off:off + 5].tolist()
    assert [v & 0xffffffff for v in got] == [0x80000000, 1, 0x807fffff, 0x00400000, 0x3f800000]
    e = packed['index'][packed['names'].index('weight')]
    w, off = packed['entries'][e]
    host = packed['healthy'][off:off + w.numel()].view(torch.float32).clone()
    back = host.as_strided(w.shape, w.stride())             # what the writer thread builds
    keep = torch.isfinite(w.cpu())
    assert back.stride() == (45, 1, 15, 5)
    assert torch.equal(back[keep], w.cpu()[keep]) and int((~keep).sum()) == 1   # (planted later)


def test_nonfinite_count_is_exact(packed):
    got, want = packed['poisoned'], packed['want_poisoned']
    assert packed['planted'] == 10
    assert int(got[1]) == 10, 'NaN / Inf planted at tensor starts, ends, chunk seams, tails'
    assert int(got[0]) == 0, 'the other header word is zeroed for the next launch'
    assert torch.equal(got, want)       # payloads preserved, gaps and the end untouched


def test_empty_input_enqueues_nothing():
    from dvs_of_training_framework_amd import _lib, snapshot
    assert _lib.lib().dvsof_snapshot_pack(None, None, None, None, 0, None, 0, None) == 0
    slab = torch.full((16,), SENTINEL, dtype=torch.int32, device=DEV)
    snapshot.pack([torch.empty(0, device=DEV)], slab)
    torch.cuda.synchronize()
    assert bool((slab == SENTINEL).all())
    assert _lib.lib().dvsof_snapshot_pack(8, 8, 8, 8, 1, slab.data_ptr() + 4, 0, None) != 0
    assert _lib.lib().dvsof_snapshot_pack(8, 8, 8, 8, 1, slab.data_ptr(), 2, None) != 0


# ---------------------------------------------------------------------------
def small_model():
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.Conv2d(8, 5, 3),
                            torch.nn.Linear(7, 3))
    return m.to(DEV).to(memory_format=torch.channels_last)


def make_optimizer(kind, model):
    from dvs_of_training_framework_amd import optim
    if kind == 'FusedAdamW':
        return optim.FusedAdamW(model.parameters(), lr=1e-2, weight_decay=1e-2, amsgrad=True)
    return getattr(optim, kind)(model.parameters(), lr=1e-2)


def some_steps(model, opt, n, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    for _ in range(n):
        for p in model.parameters():
            p.grad = torch.empty_like(p).copy_(torch.randn(p.shape, generator=g))
        opt.step()


def same_bits(a, b):
    return a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype and \
        torch.equal(storage_order(a.cpu()) if a.numel() else a.cpu(),
                    storage_order(b.cpu()) if b.numel() else b.cpu())


@pytest.mark.parametrize('kind', ['FusedAdamW', 'FusedRAdam', 'FusedRanger'])
def test_asynchronous_file_equals_the_state(tmp_path, kind, monkeypatch):
    from dvs_of_training_framework_amd.serializer import Serializer
    model = small_model()
    opt = make_optimizer(kind, model)
    some_steps(model, opt, 7)           # Ranger: past one Lookahead sync (k = 6)
    s = Serializer(tmp_path, keep_checkpoints_max=2, permanent_checkpoint_interval=0)

    # the training thread never waits for the device inside checkpoint_model
    main, guarded = threading.main_thread(), [False]

    def guard(real):
        def wrapped(*a, **k):
            if guarded[0] and threading.current_thread() is main:
                raise AssertionError('the training thread synchronised inside the hook')
            return real(*a, **k)
        return wrapped
    monkeypatch.setattr(torch.cuda, 'synchronize', guard(torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Event, 'synchronize', guard(torch.cuda.Event.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', guard(torch.cuda.Stream.synchronize))
    guarded[0] = True
    assert s.checkpoint_model(model, opt, 7, samples_passed=28) is None     # enqueued
    some_steps(model, opt, 1, seed=1)   # training goes on and overwrites the live state
    guarded[0] = False
    s.wait()
    after = {k: v.clone() for k, v in model.state_dict().items()}

    # the state at step 7, taken the slow way from an identical run
    model2 = small_model()
    opt2 = make_optimizer(kind, model2)
    some_steps(model2, opt2, 7)
    torch.cuda.synchronize()
    want_model, want_opt = model2.state_dict(), opt2.state_dict()
    file = torch.load(tmp_path / 'step_7.pt', weights_only=True)
    assert set(file) == {'model', 'optimizer', 'global_step', 'samples_passed'}
    assert file['global_step'] == 7 and file['samples_passed'] == 28
    assert list(file['model']) == list(want_model)
    for k, v in want_model.items():
        assert same_bits(file['model'][k], v), k
        assert not file['model'][k].is_cuda
    assert any(not torch.equal(after[k].cpu(), file['model'][k]) for k in after), \
        'the step after the snapshot must not leak into it'
    assert file['optimizer']['param_groups'] == want_opt['param_groups']
    assert list(file['optimizer']['state']) == list(want_opt['state'])
    for i, st in want_opt['state'].items():
        got = file['optimizer']['state'][i]
        assert list(got) == list(st)
        for name, v in st.items():
            if torch.is_tensor(v):
                assert same_bits(got[name], v), (i, name)
            else:
                assert got[name] == v == 7
        aliased = got['slow_buffer'].data_ptr() == got['exp_avg'].data_ptr() \
            if 'slow_buffer' in got else None
        assert aliased == {'FusedAdamW': None, 'FusedRAdam': True, 'FusedRanger': False}[kind]
    # each tensor owns its bytes: the file is about the size of the state
    n_bytes = sum(4 * v.numel() for v in want_model.values()) + sum(
        4 * v.numel() for st in want_opt['state'].values()
        for name, v in st.items() if torch.is_tensor(v) and not
        (kind == 'FusedRAdam' and name == 'slow_buffer'))
    assert (tmp_path / 'step_7.pt').stat().st_size < n_bytes + 32768

    # and back: a fresh optimizer continues bit for bit, the aliasing with it
    model3 = small_model()
    opt3 = make_optimizer(kind, model3)
    step, rest = s.load_checkpoint(model3, 7, optimizer=opt3, device=DEV)
    assert step == 7 and rest == {'samples_passed': 28}
    if kind == 'FusedRAdam':
        assert all(st['slow_buffer'] is st['exp_avg'] for st in opt3.state.values())
    some_steps(model3, opt3, 1, seed=1)
    torch.cuda.synchronize()
    for k, v in model3.state_dict().items():
        assert same_bits(v, after[k]), k
    s.close()


def test_tables_are_rebuilt_only_when_a_pointer_moved(tmp_path):
    from dvs_of_training_framework_amd.serializer import Serializer
    model = small_model()
    opt = make_optimizer('FusedAdamW', model)
    some_steps(model, opt, 1)
    s = Serializer(tmp_path, keep_checkpoints_max=0, permanent_checkpoint_interval=0)
    for step in (1, 2, 3):
        s.checkpoint_model(model, opt, step)
    s.wait()
    snap = s._snap
    assert (snap.launches, snap.table_builds) == (3, 1)
    dev, host = snap.dev.data_ptr(), snap.host.data_ptr()
    with torch.no_grad():
        model[2].bias.data = model[2].bias.data.clone()     # one pointer moves
    s.checkpoint_model(model, opt, 4)
    s.wait()
    assert snap.table_builds == 2
    assert (snap.dev.data_ptr(), snap.host.data_ptr()) == (dev, host)   # slabs allocated once
    assert s.list_known_steps() == [1, 2, 3, 4] and s.refused == []
    s.close()

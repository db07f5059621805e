"""``OpticalFlow`` inference wrapper with the reference's contract
(DummyNet/of.py:17-125, used by test.py:51-60): events of several windows in,
``np.ndarray [B,H,W,2]`` out."""
from os import path as osp

import numpy as np
import torch
import torch.nn as nn

from .net import Model

script_dir = osp.dirname(osp.realpath(__file__))


class OpticalFlow:
    def __init__(self, imsize, model=osp.join(script_dir, 'data/model/model.pth'),
                 device=torch.device('cuda:0'), activation=nn.ReLU(),
                 graph=False, **model_kwargs):
        # graph=True: the whole inference (voxelise + weight forms + predictor)
        # is captured once per (batch, event capacity) in a HIP graph and
        # replayed; a batch-1 call is ~50 short launches that the host cannot
        # enqueue as fast as the GPU runs them.  Events are padded to the
        # capacity with x = y = -1 (ignored by the voxeliser).
        self._use_graph, self._graphs = bool(graph), {}
        self._device = torch.device(device)
        self._net = Model(device=self._device, activation=activation,
                          **model_kwargs)
        if model is not None:
            state_dict = torch.load(model, map_location=self._device,
                                    weights_only=True)
            if 'model' in state_dict:
                state_dict = state_dict['model']
            self.load_state_dict(state_dict)
        self._net.eval()
        self.imsize = imsize

    @classmethod
    def from_model(cls, net, imsize):
        """Wrap a live ``Model`` (one that is being trained, say): no weight
        is loaded or copied, and the model's mode is the caller's business
        (``hooks.model_left_as_found``).  No graph: the weights move between
        calls."""
        self = cls.__new__(cls)
        self._use_graph, self._graphs = False, {}
        self._device = next(net.parameters()).device
        self._net = net
        self.imsize = imsize
        return self

    def load_state_dict(self, state_dict):
        self._net.load_state_dict(state_dict)
        self._net.to(device=self._device)

    def __call__(self, events, start, stop, return_all=False):
        """events: per sample (x, y, t, p) iterables, p in {-1, 1};
        start/stop: window bounds per sample."""
        with torch.no_grad():
            ev, ts, sidx = self._collate(events, start, stop)
            if self._use_graph:
                flow = self._replay(ev, ts, sidx, len(start))
            else:
                flow, _, _ = self._net(ev, ts, sidx, self.imsize)
            return self._postprocess(flow, return_all)

    def flow_device(self, events, start, stop):
        """Same arguments as ``__call__``; -> the finest flow as a DEVICE tensor
        ``[B,2,H,W]`` (the network's own layout, no copy to the host):
        what ``testing.evaluate`` hands to the error kernel."""
        with torch.no_grad():
            ev, ts, sidx = self._collate(events, start, stop)
            if self._use_graph:
                # the graph's output buffer is rewritten by the next replay
                return self._replay(ev, ts, sidx, len(start))[-1].clone()
            flow, _, _ = self._net(ev, ts, sidx, self.imsize)
            return flow[-1].contiguous()

    def _graph_slot(self, B, n, dtypes):
        """The static inputs (and, once captured, the graph) of batch size B
        with room for n events; dtypes: of the event columns."""
        g = self._graphs.get(B)
        if g is None or n > g['cap']:
            cap = max(4096, 1 << max(n - 1, 1).bit_length())
            st = {k: torch.zeros(cap, dtype=dt, device=self._device)
                  for k, dt in dtypes.items()}
            g = dict(cap=cap, ev=st,
                     ts=torch.zeros(2 * B, dtype=torch.float32, device=self._device),
                     sidx=torch.zeros(2 * B, dtype=torch.long, device=self._device),
                     graph=None, flow=None)
            self._graphs[B] = g
        return g

    def flow_sequence(self, seq, starts, stops, box=None, return_events=False):
        """The finest flow ``[F,2,H,W]`` of the frames (start_i, stop_i] of a
        device-resident ``sequence.EventSequence``, on the device like
        ``flow_device``'s; the events never visit the host: one window-kernel
        launch collates them (box = (y0, x0, h, w): cropped as by EventCrop,
        the events outside it stay in their slots as x = y = -1).  With
        graph=True the kernel writes the graph's static inputs directly and
        pads them to their capacity.  return_events: -> (flow, the collated
        batch: sequence.EventSequence.collate_frames)."""
        from .sequence import _OUT_DTYPES
        with torch.no_grad():
            B = len(starts)
            if self._use_graph:
                def static_columns(n):
                    g = self._graph_slot(B, n, _OUT_DTYPES)
                    return g['cap'], g['ev']
                c = seq.collate_frames(starts, stops, box, buffers=static_columns)
                g = self._graphs[B]
                g['ts'].copy_(c.timestamps)
                g['sidx'].copy_(c.sample_idx)
                flow = self._launch(g, B)[-1].clone()
            else:
                c = seq.collate_frames(starts, stops, box)
                flow = self._net(c.events, c.timestamps, c.sample_idx,
                                 self.imsize)[0][-1].contiguous()
            return (flow, c) if return_events else flow

    def _replay(self, ev, ts, sidx, B):
        n = ev['x'].numel()
        g = self._graph_slot(B, n, {k: v.dtype for k, v in ev.items()})
        assert ts.numel() == g['ts'].numel()
        # Replays, and the copies into the static inputs between them, are
        # ordered on one stream; no host synchronisation is needed.  The graph
        # holds kernels only (the voxeliser's control words clean up after
        # themselves, so there is no memset node; its workspace is the one the
        # eager warm-up call made).
        for k, v in ev.items():
            g['ev'][k][:n].copy_(v)
        g['ev']['x'][n:] = -1
        g['ev']['y'][n:] = -1
        g['ev']['sample_index'][n:] = 0
        g['ts'].copy_(ts)
        g['sidx'].copy_(sidx)
        return self._launch(g, B)

    def _launch(self, g, B):
        """Capture (first call) and replay the graph over the static inputs."""
        if g['graph'] is None:
            # one validated eager call (host-side assertions, lazy inits), then
            # capture without them
            self._net.strict = True
            self._net(g['ev'], g['ts'], g['sidx'], self.imsize, batch_size=B)
            self._net.strict = False
            torch.cuda.synchronize(self._device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):   # see capture.py
                g['flow'] = self._net(g['ev'], g['ts'], g['sidx'], self.imsize,
                                      batch_size=B)[0]
            g['graph'] = graph
            # eager objects the graph's kernels point at (voxeliser workspace,
            # index vectors) must outlive it whatever their caches do later
            from . import learned_voxel, voxel
            g['keep'] = (list(voxel._WORKSPACES.values()),
                         list(learned_voxel._WORKSPACES.values()),
                         dict(self._net._layout_cache))
        g['graph'].replay()
        return g['flow']

    def _collate(self, events, start, stop):
        """Stack the samples into one event dict with a sample index
        (DummyNet/of.py:76-115); timestamps are shifted to start at 0."""
        cols = {k: [] for k in ('x', 'y', 'timestamp', 'polarity',
                                'element_index', 'sample_index')}
        for i, e in enumerate(events):
            x, y, t, p = (np.asarray(v) for v in e[:4])
            cols['x'].append(x.astype(np.int64))
            cols['y'].append(y.astype(np.int64))
            cols['timestamp'].append(t.astype(np.float64))
            cols['polarity'].append(p.astype(np.int64))
            cols['element_index'].append(np.zeros(x.size, np.int64))
            cols['sample_index'].append(np.full(x.size, i, np.int64))
        timestamps = np.hstack([[b, e] for b, e in zip(start, stop)]) \
            .astype(np.float64)
        sample_idx = np.hstack([[i, i] for i in range(len(start))])
        min_t = timestamps.min()
        ev = {}
        for k, v in cols.items():
            a = np.concatenate(v) if v else np.zeros(0)
            if k == 'timestamp':
                ev[k] = torch.tensor(a - min_t, dtype=torch.float32,
                                     device=self._device)
            else:
                ev[k] = torch.tensor(a, dtype=torch.long, device=self._device)
        return ev, \
            torch.tensor(timestamps - min_t, dtype=torch.float32,
                         device=self._device), \
            torch.tensor(sample_idx, dtype=torch.long, device=self._device)

    def _postprocess(self, flow, return_all):
        def back(f):
            return np.transpose(f.detach().cpu().numpy(), (0, 2, 3, 1))
        if return_all:
            return tuple(map(back, flow))
        return back(flow[-1])

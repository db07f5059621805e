"""Every ``DVSOF_*`` environment variable the package, ``train_flownet.py`` and ``bench.py``
read: name -> (who sets it, what it does).  A variable is here because something the project
runs sets it (``bench.py``, a test, a script directly under ``tools/``), because it names a file
to load, or because it is a probe read only in the probe build; every other experiment was
retired with its result.  The call sites read the environment themselves;
this table is what tests/test_env_switches.py holds them to, and what ``report`` checks the
environment against when the package is imported.
"""
import os
import sys
from pathlib import Path

SWITCHES = {
    'DVSOF_WGRAD_STREAM': ('bench', '0: the whole backward on one stream (launch-order checks, per-launch timing)'),
    'DVSOF_DIRECT_RCCL': ('bench', "0: eager exchange through torch.distributed instead of the C ABI's communicator"),
    'DVSOF_FORCE_DIST': ('bench', '1: a one-rank process group, the RCCL path on one GPU'),
    'DVSOF_LOOPBACK': ('bench', '"world:delay_us": the loopback communicator, a late non-identity exchange on one GPU'),
    'DVSOF_LAUNCH_TIMEOUT': ('bench', "seconds before bench.py's launcher gives up on its ranks"),
    'DVSOF_FLUSH_AT': ('bench', "bench.py: other flush points of the 'coarse' update schedule"),
    'DVSOF_EAGER': ('bench', '1: bench.py runs eager steps, as --eager (sweep scripts)'),
    'DVSOF_DTYPE': ('bench', "bench.py's --dtype (sweep scripts)"),
    'DVSOF_GCONV_TILE': ('tools/tile_sweep.sh', 'tile of the general forward / data-gradient kernels'),
    'DVSOF_GCONV_K32_BLOCKS': ('tools/wino_sweep.sh', 'block count below which the v2 kernels take the K32 ring'),
    'DVSOF_WGRAD_TILE': ('tools/wgrad_sweep.sh', 'tile of the general weight-gradient kernel'),
    'DVSOF_WGRAD_SPLITS': ('tools/wgrad_sweep.sh', 'split-K factor of the general weight-gradient kernel'),
    'DVSOF_WINO_TILE': ('tools/wino_sweep.sh', 'tile of the Winograd GEMM'),
    'DVSOF_WINO_WGRAD_F': ('tools/wino_sweep.sh', 'Winograd weight gradient: F(2x2) or F(4x4)'),
    'DVSOF_WINO_WGRAD_TILE': ('tools/wino_sweep.sh', 'tile of the Winograd weight-gradient GEMM'),
    'DVSOF_WINO_WGRAD_SPLITS': ('tools/wino_sweep.sh', 'split factor of the Winograd weight-gradient GEMM'),
    'DVSOF_VOX_EPT': ('tools/gpu_vox_probe.sh', 'events per thread of the voxeliser'),
    'DVSOF_LIB_PATH': ('loader', 'path of a variant library to load instead (tools/variant.sh)'),
    'DVSOF_PROBE_LIB': ('loader', '1: load the probe build, libdvsof_hip_probes.so'),
    'DVSOF_LIBHDF5': ('loader', 'path of libhdf5 (hdf5io.py)'),
    'DVSOF_GCONV_DBG': ('probe build', 'timing-probe bits of the v2 conv kernels (results wrong by construction)'),
    'DVSOF_LOSS_DBG': ('probe build', 'timing-probe bits of the loss kernel'),
    'DVSOF_FIRST_DBG': ('probe build', "timing-probe bits of the first layer's kernel"),
    'DVSOF_FWD_PATCH_DBG': ('probe build', 'timing-probe bits of the patch-resident forward kernel'),
}


def library_path():
    """The library _lib.py loads: the product build next to the package unless
    DVSOF_LIB_PATH / DVSOF_PROBE_LIB choose another."""
    pkg = Path(__file__).resolve().parent
    if os.environ.get('DVSOF_LIB_PATH'):    # an experiment's variant build (tools/variant.sh)
        return Path(os.environ['DVSOF_LIB_PATH']).resolve()
    # the probe build (`make -C csrc probes`; the timing probes compiled in) -- diagnostics tools only
    return pkg / ('libdvsof_hip_probes.so' if os.environ.get('DVSOF_PROBE_LIB') == '1'
                  else 'libdvsof_hip.so')


def report():
    """One stderr line per DVSOF_* variable that nothing reads, one when the environment chose
    the library; otherwise silent."""
    for name in sorted(os.environ):
        if name.startswith('DVSOF_') and name not in SWITCHES:
            print(f'dvsof: {name} is set but not read (retired or misspelt)', file=sys.stderr)
    if os.environ.get('DVSOF_LIB_PATH') or os.environ.get('DVSOF_PROBE_LIB') == '1':
        print(f'dvsof: loading {library_path()}', file=sys.stderr)

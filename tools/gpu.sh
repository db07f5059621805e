#!/bin/bash
# One script for the GPU box (gpurun -- bash tools/gpu.sh <command> [args]); replaces the one-off
# scripts of earlier rounds.  Everything is written under gpurun_out/<tag>/ (tag = $TAG or the
# command name); copy what is to be kept into profiles/.
#   tests [pytest -k expression]      GPU tests (all, or a selection)
#   bench [bench.py args]             the driver's command (default) or any other bench run
#   quick [ENV=VAL ...]               short headline run (no roofline / modes / baseline) under an environment
#   conv [ENV=VAL ...]                per-launch conv table of one step, one stream
#   variants <name> [<name> ...]      `conv` under variant libraries built by tools/variant.sh
#   hbm [ENV=VAL ...]                 voxeliser / loss call paths at the BASELINE.json sizes
#   optim [optim_bench.py args]       Ranger / AdamW step, eager loop against executor replay, f32 and bf16s,
#                                     then the update and centralisation kernels alone (tools/optim_bench.py);
#                                     then its --guard leg: step guard off against on in alternating blocks,
#                                     the statistic kernels alone (docs/STEP_GUARD_SPEC.md)
#   eval [eval_bench.py args]        testing.evaluate on a synthetic MVSEC-shaped sequence: frames/s at batch 1 and 8,
#                                     the reference's per-frame structure on the host, the three kernels alone
#                                     the same frames from a device-resident EventSequence, the window kernel alone
#   evalhook [eval_bench.py args]    the evaluation hook (tools/eval_bench.py --hook): polarity count and the panel
#                                     launch pair alone at F = 8, 256x256, against the numpy restatement on the host;
#                                     one hook call over 200 frames against the step time of the same run
#   iwe [iwe_bench.py args]          label-free validation (tools/iwe_bench.py): splat, statistics and render alone at
#                                     F = 8, 256x256, 30 000 and 120 000 events per frame, the splat's atomic bytes/s;
#                                     testing.flow_warp_loss against the same frames' inference alone;
#                                     dvsof_iwe_splat_multi at masks 1, 5, 7 without and with polarity and, at mask 1
#                                     without, against count image + splat; --references / --polarity: the metric there
#   contrast [contrast_bench.py args] contrast-maximisation term (tools/contrast_bench.py): dvsof_contrast_fwd and
#                                     dvsof_contrast_bwd alone at batch 8, 256x256, 65 536 events per sample; the eager
#                                     training step with --contrast-weight 0 against 0.25 in alternating blocks
#   contrast-multi [contrast_bench.py args]  its --multi leg: dvsof_contrast_fwd / _bwd, dvsof_contrast_multi_fwd /
#                                     _bwd at mask = start without polarity (the same kernels of csrc/contrast.hip
#                                     through the general entry point) and at all three references with polarity, in
#                                     alternating blocks of one run (profiles/contrast_multi/README.md)
#   contrast_pyramid [contrast_pyramid_bench.py args]  the term on every flow scale (tools/contrast_pyramid_bench.py):
#                                     dvsof_contrast_pyramid_fwd / _bwd against four calls of dvsof_contrast_multi_fwd /
#                                     _bwd on shifted columns at batch 8, 256x256, four levels, what a level costs alone,
#                                     and one eager Ranger step of a frameless batch with --contrast-scales all against
#                                     finest, in alternating blocks of one run (profiles/contrast_pyramid/README.md)
#   frameless [frameless_bench.py args]  the loss that reads no frame (tools/frameless_bench.py): dvsof_loss_frameless
#                                     against dvsof_loss_fused_pyramid on zero frames with photometric weight 0 at
#                                     batch 8, 256x256, four scales, and one eager Ranger step of a frameless batch
#                                     against the framed one with zero images, in alternating blocks of one run
#                                     (profiles/frameless/README.md)
#   avgts [avg_timestamp_bench.py args]  the average-timestamp term (tools/avg_timestamp_bench.py): dvsof_avg_timestamp_fwd /
#                                     _bwd against dvsof_contrast_multi_fwd / _bwd at start,end and at start,middle,end
#                                     with polarity, batch 8, 256x256, 65 536 events per sample, and one eager Ranger
#                                     step with and without --avg-timestamp-weight, in alternating blocks of one run
#                                     (profiles/avg_timestamp/README.md)
#   avgts_pyramid [avg_timestamp_bench.py args]  that term on every flow scale (its --scales all legs):
#                                     dvsof_avg_timestamp_pyramid_fwd / _bwd against four calls of dvsof_avg_timestamp_fwd /
#                                     _bwd on shifted columns at batch 8, 256x256, four levels, start,end with and without
#                                     polarity, the launches of either counted from a capture, and one eager Ranger step
#                                     of a frameless batch with --avg-timestamp-scales all against finest, in alternating
#                                     blocks of one run (profiles/avg_timestamp_pyramid/README.md)
#   eventcapture [event_terms_capture_bench.py args]  the captured step with the events-only terms
#                                     (--capture-event-terms; tools/event_terms_capture_bench.py): framed + contrast,
#                                     frameless + contrast on every scale, the same + average timestamp, f32 and bf16s,
#                                     eager loop against executor replay in alternating blocks of one run after a
#                                     bitwise comparison of the two (profiles/event_terms_capture/README.md)
#   eventencoded [event_terms_encoded_bench.py args]  the events-only terms on the 9 B/event encoded columns
#                                     (--compact-event-terms; tools/event_terms_encoded_bench.py): the eight encoded
#                                     entry points against their wire twins after a bitwise comparison, and the train
#                                     loop fed through feed.DeviceFeeder with the contrast term on every scale, compact
#                                     against wire batches, eager and replayed, in alternating blocks of one run; on a
#                                     commit without the entry points the wire legs alone
#                                     (profiles/event_terms_encoded/README.md)
#   learned [learned_voxel_bench.py args]  learnable representation: forward against the fixed voxeliser, table gradient,
#                                     enc.0 data gradient, eager step with and without it, executor replay of the
#                                     resident model against its eager loop, the same under DVSOF_LOOPBACK=8:50;
#                                     forward_alternating: float-atomics forward / learned_fwd_deterministic /
#                                     fixed voxeliser in alternating blocks of one run
#                                     (tools/learned_voxel_bench.py)
#   checkpoint [checkpoint_bench.py args]  training-thread stall of a reference-style checkpoint against the device
#                                     snapshot + writer thread, the gather launch alone, samples/s with a checkpoint
#                                     every 100 steps against none (tools/checkpoint_bench.py)
#   lossprobe B H W bits...           loss path under the probe build's DVSOF_LOSS_DBG bits
#   timeline [bench args]             rocprofv3 kernel trace of a short run -> one step per queue
#   feedtrace [wire|compact]          kernel + memory-copy trace of the train loop fed from host memory
#   nodes [bench args]                the executor's plan (lane, stand-alone us of every kernel)
#   collect <stage>                   everything under profiles/<round>/: tools/collect_profiles.sh +
#                                     HBM-path PMC passes + plan + timeline + loopback / 1-rank-group runs
#   rccl2                             does RCCL accept two ranks on one GPU? (it does not)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
R=$PWD; cmd=${1:-tests}; shift
O=$R/gpurun_out/${TAG:-$cmd}; mkdir -p $O
envs=(); while [[ "$1" == *=* && "$1" != -* ]]; do envs+=("$1"); shift; done
short="--steps 30 --warmup 5 --no-roofline --no-other-modes --no-cpu-baseline --no-train-loop"
case $cmd in
tests)
  if [ -n "$1" ]; then timeout -k 10 1100 python -m pytest tests -x -q -m gpu -k "$1" > $O/pytest.txt 2>&1
  else timeout -k 10 1100 python -m pytest tests -x -q -m gpu > $O/pytest.txt 2>&1; fi
  echo "pytest rc=$?"; tail -8 $O/pytest.txt ;;
bench)
  timeout -k 10 900 env "${envs[@]}" python bench.py "$@" > $O/bench.json 2> $O/bench.err; echo "bench rc=$?"
  python - $O/bench.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d['value'], d['unit'], d['ms_per_step'], 'ms |', d['config'].get('launch', '')[:90])
r = d.get('roofline')
if r: print(r['kernel'], r['achieved'], r['frac'], '| step', r['step'])
PY
  ;;
quick)
  timeout -k 10 600 env "${envs[@]}" python bench.py $short "$@" 2> $O/quick.err | tee $O/quick.json | python -c "import json,sys;d=json.loads(sys.stdin.read());print(d['value'], d['ms_per_step'])" ;;
conv)
  timeout -k 10 300 env DVSOF_WGRAD_STREAM=0 "${envs[@]}" python tools/conv_bench.py "$@" > $O/conv.txt 2>&1; cat $O/conv.txt ;;
variants)
  for v in base "$@"; do
    lib=; [ $v != base ] && lib=DVSOF_LIB_PATH=dvs_of_training_framework_amd/csrc/variants/$v/libdvsof_hip.so
    echo "== $v"; timeout -k 10 300 env DVSOF_WGRAD_STREAM=0 $lib python tools/conv_bench.py 2>&1 | awk '$6==1 {printf "%s %s | ", $1, $8} END{print ""}'
  done ;;
hbm)
  timeout -k 10 300 env "${envs[@]}" python tools/hbm_bench.py 2>&1 | tee $O/hbm.txt ;;
optim)
  timeout -k 10 840 env "${envs[@]}" python tools/optim_bench.py "$@" > $O/optim.jsonl 2> $O/optim.err
  rc=$?; echo "optim rc=$rc"; cut -c1-420 $O/optim.jsonl; tail -3 $O/optim.err
  [ $rc -eq 0 ] || exit $rc       # nothing more on the GPU after a failed leg
  timeout -k 10 560 env "${envs[@]}" python tools/optim_bench.py --guard "$@" > $O/optim_guard.jsonl 2> $O/optim_guard.err
  echo "optim guard rc=$?"; cut -c1-420 $O/optim_guard.jsonl; tail -3 $O/optim_guard.err ;;
eval)
  timeout -k 10 560 env "${envs[@]}" python tools/eval_bench.py "$@" > $O/eval.json 2> $O/eval.err
  echo "eval rc=$?"; cut -c1-2600 $O/eval.json; tail -3 $O/eval.err ;;
evalhook)
  timeout -k 10 560 env "${envs[@]}" python tools/eval_bench.py --hook "$@" > $O/eval_hook.json 2> $O/eval_hook.err
  echo "evalhook rc=$?"; cut -c1-2600 $O/eval_hook.json; tail -3 $O/eval_hook.err ;;
iwe)
  timeout -k 10 560 env "${envs[@]}" python tools/iwe_bench.py "$@" > $O/iwe.json 2> $O/iwe.err
  echo "iwe rc=$?"; cut -c1-2600 $O/iwe.json; tail -3 $O/iwe.err ;;
contrast)
  timeout -k 10 420 env "${envs[@]}" python tools/contrast_bench.py "$@" > $O/contrast.json 2> $O/contrast.err
  echo "contrast rc=$?"; cut -c1-2600 $O/contrast.json; tail -3 $O/contrast.err ;;
contrast-multi)
  timeout -k 10 420 env "${envs[@]}" python tools/contrast_bench.py --multi "$@" > $O/contrast_multi.json 2> $O/contrast_multi.err
  echo "contrast-multi rc=$?"; cut -c1-2600 $O/contrast_multi.json; tail -3 $O/contrast_multi.err ;;
contrast_pyramid)
  timeout -k 10 540 env "${envs[@]}" python tools/contrast_pyramid_bench.py "$@" > $O/contrast_pyramid.json 2> $O/contrast_pyramid.err
  echo "contrast_pyramid rc=$?"; cut -c1-3600 $O/contrast_pyramid.json; tail -3 $O/contrast_pyramid.err ;;
frameless)
  timeout -k 10 420 env "${envs[@]}" python tools/frameless_bench.py "$@" > $O/frameless.json 2> $O/frameless.err
  echo "frameless rc=$?"; cut -c1-2600 $O/frameless.json; tail -3 $O/frameless.err ;;
avgts)
  timeout -k 10 540 env "${envs[@]}" python tools/avg_timestamp_bench.py "$@" > $O/avgts.json 2> $O/avgts.err
  echo "avgts rc=$?"; cut -c1-3600 $O/avgts.json; tail -3 $O/avgts.err ;;
avgts_pyramid)
  timeout -k 10 540 env "${envs[@]}" python tools/avg_timestamp_bench.py --scales all "$@" > $O/avgts_pyramid.json 2> $O/avgts_pyramid.err
  echo "avgts_pyramid rc=$?"; cut -c1-4800 $O/avgts_pyramid.json; tail -3 $O/avgts_pyramid.err ;;
eventcapture)
  timeout -k 10 560 env "${envs[@]}" python tools/event_terms_capture_bench.py "$@" > $O/eventcapture.jsonl 2> $O/eventcapture.err
  echo "eventcapture rc=$?"; cut -c1-900 $O/eventcapture.jsonl; tail -3 $O/eventcapture.err ;;
eventencoded)
  timeout -k 10 560 env "${envs[@]}" python tools/event_terms_encoded_bench.py "$@" > $O/eventencoded.jsonl 2> $O/eventencoded.err
  echo "eventencoded rc=$?"; cut -c1-700 $O/eventencoded.jsonl; tail -3 $O/eventencoded.err ;;
learned)
  timeout -k 10 420 env "${envs[@]}" python tools/learned_voxel_bench.py "$@" > $O/learned.json 2> $O/learned.err
  rc=$?; echo "learned rc=$rc"; cut -c1-2000 $O/learned.json; tail -3 $O/learned.err
  [ $rc -eq 0 ] || exit $rc       # nothing more on the GPU after a failed leg
  # the resident model's replay against its eager loop under the loopback exchange (8 ranks, 50 us)
  timeout -k 10 300 env "${envs[@]}" DVSOF_LOOPBACK=8:50 python tools/learned_voxel_bench.py --captured-only "$@" > $O/learned_loopback.json 2> $O/learned_loopback.err
  echo "learned loopback rc=$?"; cut -c1-2000 $O/learned_loopback.json; tail -3 $O/learned_loopback.err ;;
checkpoint)
  timeout -k 10 560 env "${envs[@]}" python tools/checkpoint_bench.py "$@" > $O/checkpoint.jsonl 2> $O/checkpoint.err
  echo "checkpoint rc=$?"; cut -c1-600 $O/checkpoint.jsonl; tail -3 $O/checkpoint.err ;;
lossprobe)
  B=$1; H=$2; W=$3; shift 3
  for bits in "$@"; do echo -n "DBG=$bits: "; DVSOF_LOSS_DBG=$bits DVSOF_PROBE_LIB=1 timeout -k 10 120 python tools/loss_probe.py $B $H $W 2>&1 | tail -1; done ;;
timeline)
  cd /tmp && export TMPDIR=/tmp
  rocprofv3 --kernel-trace --output-format csv -d $O/t -o t -- python3 $R/bench.py --steps 12 --warmup 3 --no-cpu-baseline --no-other-modes --no-roofline --no-train-loop "$@" > $O/trace.log 2>&1 || { tail -3 $O/trace.log; exit 1; }
  cd $R; python3 tools/timeline.py $(find $O/t -name "*kernel_trace.csv") > $O/timeline.txt; rm -rf $O/t; head -4 $O/timeline.txt ;;
feedtrace)
  leg=${1:-wire}
  timeout -k 10 300 python3 tools/feed_trace.py $leg 90 > $O/plain_$leg.json 2> $O/plain.err || { tail -3 $O/plain.err; exit 1; }
  cat $O/plain_$leg.json; echo
  cd /tmp && export TMPDIR=/tmp
  rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $O/t -o t -- python3 $R/tools/feed_trace.py $leg 45 > $O/trace.log 2>&1 || { tail -3 $O/trace.log; exit 1; }
  cd $R; python3 tools/feed_timeline.py $O/t > $O/feed_$leg.txt; rm -rf $O/t; head -40 $O/feed_$leg.txt ;;
nodes)
  python3 tools/exec_nodes.py "$@" | tee $O/exec_nodes.txt | tail -3 ;;
collect)
  bash tools/collect_round.sh ;;
rccl2)
  timeout -k 10 200 python tools/rccl_share_gpu.py 2>&1 | grep -v "^$" | tail -8 ;;
*) echo "unknown command $cmd"; exit 2 ;;
esac

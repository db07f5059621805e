// Step executor: a captured training (or inference) step replayed as PLAIN
// kernel launches from one C call.
//
// The loop body of the reference (utils/training.py:138-167) is ~120 kernel
// launches here.  Enqueued from Python it costs the host ~2 ms per step
// (ctypes + descriptor building, ~17 us per launch); replayed by
// hipGraphLaunch the host is free, but ROCm 7.2's graph runtime re-schedules
// the two backward branches onto its own queues (the hand-tuned two-stream
// overlap is lost: 3.47 vs 3.24 ms of GPU time per step).  This
// executor keeps the capture -- one recording of the step for a batch
// signature -- and drops the graph runtime: it reads the kernel nodes and the
// edges of the captured hipGraph, splits the nodes into "lanes" (one per HIP
// stream), and replays them in capture order with hipLaunchKernel, an event
// per edge that crosses lanes.  Same kernels, same arguments, same order as
// the eager step: bit-identical results, the two-stream overlap, and a host
// cost of a bare launch call per kernel.
//
// Two files.  exec_sched.h DECIDES, in standard C++ that runs without a GPU
// (tools/exec_sched_check.cpp): the capture order, the greedy chain split, the
// exchange windows, the rewrite that lets kernels bypass BUCKET marks, the
// update lane, the three lane plans, and wire(), which turns a plan into
// cross-lane waits.  This file is the HIP side: it reads the hipGraph into
// exec_sched::Nodes, owns the events the wiring asks for, launches, times the
// calibration pass and the plan trials, and implements the C ABI.  Nodes are
// held by capture id and never move; the launch loop walks the plan's order.
//
// Lanes.  A dependency that crosses queues costs the consumer ~13 us after the
// producer has ended (measured; same queue: 0-7 us), so the chain that bounds
// the step must never change queues.  dvsof_exec_calibrate runs the step once
// on ONE stream with a timing event between kernels; lane 0 (the caller's
// stream) is then the longest path of the DAG by measured time, lane 1 the
// longest path among the remaining nodes, ..., the last lane takes whatever
// is left, in capture order.  Before calibration a greedy chain split is used
// (extend the chain of a dependency that is still the tail of its lane).
//
// The graph must consist of kernel nodes (and empty nodes); it has to stay
// alive while the executor is (kernel arguments are read from the nodes).
//
// Data parallelism.  The gradient exchange is not a kernel of ours: while a
// step is captured parallel.GradReducer leaves MARKS in the capture instead
// of collectives (dvsof_exec_mark: a one-thread no-op kernel whose arguments
// name the bucket).  The executor recognises the marks by their function
// address and never launches them: a BUCKET mark becomes "record an event on
// the lane that closed the bucket, make the exchange stream wait for it,
// ncclAllReduce (average, in place) on the exchange stream"; the JOIN mark in
// front of the optimizer becomes "the lane waits for the exchange stream".
// Same collectives in the same order on every rank (the launch order is a
// property of the captured graph, identical across replicas).  Without a
// communicator (dvsof_exec_set_comm not called: one GPU) marks are skipped.
#include "common.h"
#include "exec_sched.h"
#include <string.h>
#include <unordered_map>

namespace {

using namespace exec_sched;

// kind: DVSOF_MARK_BUCKET / DVSOF_MARK_JOIN.  Never runs under the executor;
// under hipGraphLaunch it is a no-op (and the exchange is then missing: the
// captured step refuses that combination).
__global__ void exec_mark_kernel(int kind, int index, float *bucket, size_t n) {}

// What the launch of a node needs; kind, dependencies and lanes are the scheduler's.
struct XNode {
    hipKernelNodeParams kp;
    float *mark_ptr = nullptr;
    size_t mark_n = 0;
    hipEvent_t mark_ev = nullptr;   // BUCKET: the lane's progress the exchange stream waits for
    hipEvent_t xdone_ev = nullptr;  // BUCKET: the exchange stream's progress behind this collective
    hipEvent_t ev = nullptr;        // recorded after the launch when another lane waits for it
};

struct Exec {
    std::vector<XNode> nodes;    // by capture id
    Sched s;
    Plan plan;                   // in effect
    Wiring w;                    // of `plan` and the streams set
    std::vector<Plan> cands;     // plans being tried on the steps after calibration
    std::vector<float> best_us;  // fastest measured step under each of them
    int trial_next = -1;         // next trial (round-robin over cands), -1: settled
    int trial_cur = -1;          // plan of the step in flight whose time is still to be read
    hipEvent_t t0 = nullptr, t1 = nullptr;
    std::vector<hipStream_t> side;   // lanes 1.. (lane 0 is the stream of the launch call)
    hipEvent_t fork = nullptr;
    std::vector<hipEvent_t> join;    // per side lane
    int n_kernels = 0, n_marks = 0;
    void *comm = nullptr;            // dvsof_comm_create handle (not owned)
    hipStream_t xstream = nullptr;   // exchange stream (not owned)
    hipEvent_t xdone = nullptr;      // exchange stream's progress at a JOIN mark
    hipStream_t ustream = nullptr;   // UPDATE stream: lane of the update nodes (own stream: on the exchange
                                     // stream the updates would sit between the collectives -- under the
                                     // loopback exchange that stream is the step's longest chain)
};

// Wires the plan in effect and creates the events that wiring needs (an event made for an
// earlier wiring stays until the executor goes: a step in flight may still refer to it).
int rewire(Exec *x)
{
    x->w = wire(x->s, x->plan, x->comm && x->xstream && x->ustream);
    for (size_t i = 0; i < x->nodes.size(); ++i)
        if (x->w.need_event[i] && !x->nodes[i].ev)
            DVSOF_HIP_TRY(hipEventCreateWithFlags(&x->nodes[i].ev, hipEventDisableTiming));
    if (x->w.n_lanes > 1 && !x->fork) DVSOF_HIP_TRY(hipEventCreateWithFlags(&x->fork, hipEventDisableTiming));
    while ((int)x->join.size() < x->w.n_lanes - 1) {
        hipEvent_t e;
        DVSOF_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        x->join.push_back(e);
    }
    return DVSOF_OK;
}

int use(Exec *x, const Plan &p)
{
    x->plan = p;
    return rewire(x);
}

void destroy(Exec *x)
{
    for (auto &n : x->nodes) {
        if (n.ev) (void)hipEventDestroy(n.ev);
        if (n.mark_ev) (void)hipEventDestroy(n.mark_ev);
        if (n.xdone_ev) (void)hipEventDestroy(n.xdone_ev);
    }
    if (x->xdone) (void)hipEventDestroy(x->xdone);
    if (x->t0) (void)hipEventDestroy(x->t0);
    if (x->t1) (void)hipEventDestroy(x->t1);
    if (x->fork) (void)hipEventDestroy(x->fork);
    for (auto e : x->join)
        if (e) (void)hipEventDestroy(e);
    delete x;
}

int launch_node(const XNode &n, hipStream_t st)
{
    if (n.kp.kernelParams) {
        DVSOF_HIP_TRY(hipLaunchKernel(n.kp.func, n.kp.gridDim, n.kp.blockDim, n.kp.kernelParams,
                                      n.kp.sharedMemBytes, st));
    } else {
        DVSOF_HIP_TRY(hipModuleLaunchKernel((hipFunction_t)n.kp.func, n.kp.gridDim.x, n.kp.gridDim.y,
                                            n.kp.gridDim.z, n.kp.blockDim.x, n.kp.blockDim.y,
                                            n.kp.blockDim.z, n.kp.sharedMemBytes, st, nullptr,
                                            n.kp.extra));
    }
    return DVSOF_OK;
}

// The mark `id` at its place in the launch order, on the stream `st` of its lane.
int run_mark(Exec *x, int id, hipStream_t st)
{
    if (!x->comm) return DVSOF_OK;   // one GPU: nothing to exchange
    const XNode &n = x->nodes[id];
    const int kind = x->s.nodes[id].kind;
    hipStream_t xs = x->xstream ? x->xstream : st;
    if (kind == BUCKET) {
        if (xs != st) {
            DVSOF_HIP_TRY(hipEventRecord(n.mark_ev, st));
            DVSOF_HIP_TRY(hipStreamWaitEvent(xs, n.mark_ev, 0));
        }
        const int rc = dvsof_allreduce_bucket(x->comm, n.mark_ptr, n.mark_n, (void *)xs);
        if (rc) return rc;
        if (xs != st && x->w.xdone_used[id]) DVSOF_HIP_TRY(hipEventRecord(n.xdone_ev, xs));
        return DVSOF_OK;
    }
    if (kind == WAIT) {
        const int b = x->w.wait_for[id];
        if (xs != st && b >= 0) DVSOF_HIP_TRY(hipStreamWaitEvent(st, x->nodes[b].xdone_ev, 0));
        return DVSOF_OK;
    }
    if (kind == JOIN && xs != st) {
        DVSOF_HIP_TRY(hipEventRecord(x->xdone, xs));
        DVSOF_HIP_TRY(hipStreamWaitEvent(st, x->xdone, 0));
    }
    return DVSOF_OK;
}

void copy_name(char *dst, int len, const char *s)
{
    if (!dst || len <= 0) return;
    int k = 0;
    for (; k < len - 1 && s[k]; ++k) dst[k] = s[k];
    dst[k] = 0;
}

}  // namespace

extern "C" {

int dvsof_exec_mark(int kind, int index, float *bucket, size_t n, void *stream)
{
    if (kind != DVSOF_MARK_BUCKET && kind != DVSOF_MARK_JOIN && kind != DVSOF_MARK_WAIT) return DVSOF_EINVAL;
    if (kind == DVSOF_MARK_BUCKET && (!bucket || n == 0)) return DVSOF_EINVAL;
    hipLaunchKernelGGL(exec_mark_kernel, dim3(1), dim3(1), 0, as_stream(stream), kind, index, bucket, n);
    DVSOF_LAUNCH_CHECK();
    return DVSOF_OK;
}

int dvsof_exec_set_comm(void *exec, void *comm, void *exchange_stream)
{
    if (!exec) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    x->comm = comm;
    x->xstream = as_stream(exchange_stream);
    if (comm && !x->xdone) DVSOF_HIP_TRY(hipEventCreateWithFlags(&x->xdone, hipEventDisableTiming));
    // (without dvsof_exec_set_update_stream the updates go on the exchange stream itself, between
    // the collectives)
    if (comm && x->xstream && !x->ustream) x->ustream = x->xstream;
    for (size_t i = 0; i < x->nodes.size(); ++i) {
        XNode &n = x->nodes[i];
        if (comm && x->s.nodes[i].kind == BUCKET && !n.mark_ev) {
            DVSOF_HIP_TRY(hipEventCreateWithFlags(&n.mark_ev, hipEventDisableTiming));
            DVSOF_HIP_TRY(hipEventCreateWithFlags(&n.xdone_ev, hipEventDisableTiming));
        }
    }
    return rewire(x);   // the update lane exists from here on
}

int dvsof_exec_set_update_stream(void *exec, void *update_stream)
{
    if (!exec || !update_stream) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    x->ustream = as_stream(update_stream);
    return rewire(x);
}

int dvsof_exec_marks(void *exec, int *n_marks)
{
    if (!exec || !n_marks) return DVSOF_EINVAL;
    *n_marks = ((Exec *)exec)->n_marks;
    return DVSOF_OK;
}

int dvsof_exec_mark_window(void *exec, int k, float **bucket, size_t *n, int *index, int *nodes, int cap,
                           int *count)
{
    if (!exec || k < 0 || !count || cap < 0 || (cap > 0 && !nodes)) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    int m = -1;     // the k-th BUCKET mark in capture order
    for (int i = 0; i < (int)x->nodes.size() && m < 0; ++i)
        if (x->s.nodes[i].kind == BUCKET && k-- == 0) m = i;
    if (m < 0) return DVSOF_EINVAL;
    if (bucket) *bucket = x->nodes[m].mark_ptr;
    if (n) *n = x->nodes[m].mark_n;
    if (index) *index = x->s.nodes[m].mark_index;
    const std::vector<int> &win = x->s.window[m];
    *count = (int)win.size();
    for (int j = 0; j < *count && j < cap; ++j) nodes[j] = x->w.pos[win[j]];
    return DVSOF_OK;
}

int dvsof_exec_node_arg(void *exec, int i, int arg, size_t nbytes, void *out)
{
    if (!exec || !out) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    if (i < 0 || i >= (int)x->nodes.size() || arg < 0) return DVSOF_EINVAL;
    const int id = x->plan.order[i];
    const XNode &n = x->nodes[id];
    if (x->s.nodes[id].kind == EMPTY || !n.kp.kernelParams || !n.kp.kernelParams[arg]) return DVSOF_EINVAL;
    memcpy(out, n.kp.kernelParams[arg], nbytes);
    return DVSOF_OK;
}

int dvsof_exec_create(void *graph_, void *const *side_streams, int n_side, void **out)
{
    if (!graph_ || !out || n_side < 0 || (n_side > 0 && !side_streams)) return DVSOF_EINVAL;
    hipGraph_t graph = (hipGraph_t)graph_;
    size_t nn = 0, ne = 0;
    DVSOF_HIP_TRY(hipGraphGetNodes(graph, nullptr, &nn));
    if (nn == 0) return DVSOF_EINVAL;
    std::vector<hipGraphNode_t> hn(nn);
    DVSOF_HIP_TRY(hipGraphGetNodes(graph, hn.data(), &nn));
    DVSOF_HIP_TRY(hipGraphGetEdges(graph, nullptr, nullptr, &ne));
    std::vector<hipGraphNode_t> ef(ne), et(ne);
    if (ne) DVSOF_HIP_TRY(hipGraphGetEdges(graph, ef.data(), et.data(), &ne));

    std::unordered_map<hipGraphNode_t, int> raw_index;
    for (size_t i = 0; i < nn; ++i) raw_index[hn[i]] = (int)i;
    auto index_of = [&](hipGraphNode_t h) {     // -1: not a node of the graph (topo_order refuses it)
        auto it = raw_index.find(h);
        return it == raw_index.end() ? -1 : it->second;
    };
    std::vector<std::pair<int, int>> edges(ne);
    for (size_t e = 0; e < ne; ++e) edges[e] = {index_of(ef[e]), index_of(et[e])};
    std::vector<int> order;
    std::vector<std::vector<int>> deps;
    if (!topo_order((int)nn, edges, order, deps)) return DVSOF_EINVAL;

    Exec *x = new Exec;
    x->nodes.resize(nn);
    std::vector<Node> nodes(nn);
    auto fail = [&](int rc) {
        destroy(x);
        return rc;
    };
    for (size_t i = 0; i < nn; ++i) {
        XNode &n = x->nodes[i];
        const hipGraphNode_t h = hn[order[i]];
        nodes[i].deps = deps[i];
        hipGraphNodeType ty;
        hipError_t e = hipGraphNodeGetType(h, &ty);
        if (e != hipSuccess) return fail((int)e);
        if (ty == hipGraphNodeTypeKernel) {
            e = hipGraphKernelNodeGetParams(h, &n.kp);
            if (e != hipSuccess) return fail((int)e);
            if (!n.kp.func || (!n.kp.kernelParams && !n.kp.extra)) return fail(DVSOF_EINVAL);
            if (n.kp.func == (void *)exec_mark_kernel && n.kp.kernelParams) {
                nodes[i].kind = *(const int *)n.kp.kernelParams[0];
                nodes[i].mark_index = *(const int *)n.kp.kernelParams[1];
                n.mark_ptr = *(float *const *)n.kp.kernelParams[2];
                n.mark_n = *(const size_t *)n.kp.kernelParams[3];
                ++x->n_marks;
            } else {
                ++x->n_kernels;
            }
        } else if (ty == hipGraphNodeTypeEmpty) {
            nodes[i].kind = EMPTY;
        } else {
            return fail(DVSOF_EINVAL);      // memset / memcpy / host nodes: not a kernels-only step
        }
    }
    x->s = build(std::move(nodes), 1 + n_side);
    for (int l = 0; l < n_side; ++l) x->side.push_back((hipStream_t)side_streams[l]);
    const int rc = use(x, plan_chain(x->s));
    if (rc) return fail(rc);
    *out = x;
    return DVSOF_OK;
}

int dvsof_exec_info(void *exec, int *n_kernels, int *n_lanes, int *n_events, int *n_waits,
                    int *lane_kernels, int max_lanes)
{
    if (!exec) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    if (n_kernels) *n_kernels = x->n_kernels;
    if (n_lanes) *n_lanes = x->w.n_lanes;
    if (n_events) *n_events = x->w.n_events;
    if (n_waits) *n_waits = x->w.n_waits;
    if (lane_kernels) {
        for (int l = 0; l < max_lanes; ++l) lane_kernels[l] = 0;
        for (size_t i = 0; i < x->nodes.size(); ++i)
            if (x->s.nodes[i].kind == KERNEL && x->w.lane[i] < max_lanes) ++lane_kernels[x->w.lane[i]];
    }
    return DVSOF_OK;
}

int dvsof_exec_node(void *exec, int i, int *lane, float *us, int *n_waits, char *name, int name_len)
{
    if (!exec) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    if (i < 0 || i >= (int)x->nodes.size()) return DVSOF_EINVAL;
    const int id = x->plan.order[i];
    const XNode &n = x->nodes[id];
    if (lane) *lane = x->w.lane[id];
    if (us) *us = x->s.nodes[id].us;
    if (n_waits) *n_waits = (int)x->w.wait[id].size();
    const bool empty = x->s.nodes[id].kind == EMPTY;
    const char *s = !empty && n.kp.kernelParams ? hipKernelNameRefByPtr(n.kp.func, nullptr) : nullptr;
    copy_name(name, name_len, s ? s : empty ? "(empty)" : "?");
    return DVSOF_OK;
}

int dvsof_exec_calibrate(void *exec, void *stream)
{
    if (!exec) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    hipStream_t st = as_stream(stream);
    const int nn = (int)x->nodes.size();
    std::vector<hipEvent_t> ev(nn + 1, nullptr);
    auto run = [&]() -> int {
        for (auto &e : ev) DVSOF_HIP_TRY(hipEventCreate(&e));
        DVSOF_HIP_TRY(hipEventRecord(ev[0], st));
        for (int i = 0; i < nn; ++i) {
            const int id = x->plan.order[i], kind = x->s.nodes[id].kind;
            const XNode &n = x->nodes[id];
            int rc_ = DVSOF_OK;
            if (kind == KERNEL)
                rc_ = launch_node(n, st);
            else if (kind == BUCKET && x->comm)     // the exchange in stream order on the one stream of this pass
                rc_ = dvsof_allreduce_bucket(x->comm, n.mark_ptr, n.mark_n, (void *)st);
            if (rc_) return rc_;
            DVSOF_HIP_TRY(hipEventRecord(ev[i + 1], st));
        }
        DVSOF_HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < nn; ++i) {
            float ms = 0.f;
            DVSOF_HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            Node &n = x->s.nodes[x->plan.order[i]];
            n.us = n.kind == KERNEL ? std::max(ms * 1e3f, 0.5f) : 0.f;
        }
        return DVSOF_OK;
    };
    const int rc = run();
    for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc) return rc;
    // every plan is tried on the next steps (real steps, timed on the device), the fastest stays
    constexpr double hop = 8.0;
    x->cands.clear();
    x->trial_next = x->trial_cur = -1;
    if (x->s.max_lanes < 2) return rewire(x);
    // Under an exchange every rank takes the SAME plan, the capture's own two-stream split
    // ("chain": what the trials picked in every 1-rank and loopback run): timed trials would
    // measure the other ranks' arrival at the collectives as much as this rank's kernels, ranks
    // could settle on different plans, and the trial steps themselves (host waits for a step's
    // end) are one more place where ranks wait for each other.
    if (x->comm) return use(x, plan_chain(x->s));
    x->cands = {plan_paths(x->s), plan_list(x->s, hop), plan_chain(x->s)};
    x->best_us.assign(x->cands.size(), 3.0e38f);
    if (!x->t0) DVSOF_HIP_TRY(hipEventCreate(&x->t0));
    if (!x->t1) DVSOF_HIP_TRY(hipEventCreate(&x->t1));
    x->trial_next = 0;
    return use(x, x->cands[0]);
}

// Steps after calibration: plan k % n on trial k, `rounds` rounds; then the fastest.
static int next_trial(Exec *x)
{
    constexpr int rounds = 2;
    const int n = (int)x->cands.size();
    if (x->trial_cur >= 0) {    // the step in flight was a trial: its device time
        DVSOF_HIP_TRY(hipEventSynchronize(x->t1));
        float ms = 0.f;
        DVSOF_HIP_TRY(hipEventElapsedTime(&ms, x->t0, x->t1));
        x->best_us[x->trial_cur] = std::min(x->best_us[x->trial_cur], ms * 1e3f);
        x->trial_cur = -1;
    }
    if (x->trial_next < n * rounds) {
        x->trial_cur = x->trial_next++ % n;
        return use(x, x->cands[x->trial_cur]);
    }
    x->trial_next = -1;
    return use(x, x->cands[std::min_element(x->best_us.begin(), x->best_us.end()) - x->best_us.begin()]);
}

int dvsof_exec_launch(void *exec, void *stream)
{
    if (!exec) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    hipStream_t main = as_stream(stream);
    if (x->trial_next >= 0) {
        const int rc_ = next_trial(x);
        if (rc_) return rc_;
    }
    const int L = x->w.n_lanes;
    auto lane_stream = [&](int l) { return l == 0 ? main : l <= (int)x->side.size() ? x->side[l - 1] : x->ustream; };
    if (x->trial_cur >= 0) DVSOF_HIP_TRY(hipEventRecord(x->t0, main));
    if (L > 1) {   // the side lanes start behind whatever precedes the step on `stream`
        DVSOF_HIP_TRY(hipEventRecord(x->fork, main));
        for (int l = 1; l < L; ++l) DVSOF_HIP_TRY(hipStreamWaitEvent(lane_stream(l), x->fork, 0));
    }
    for (int id : x->plan.order) {
        const XNode &n = x->nodes[id];
        const int kind = x->s.nodes[id].kind;
        hipStream_t st = lane_stream(x->w.lane[id]);
        for (int d : x->w.wait[id]) DVSOF_HIP_TRY(hipStreamWaitEvent(st, x->nodes[d].ev, 0));
        const int rc_ = kind == KERNEL ? launch_node(n, st) : is_mark(kind) ? run_mark(x, id, st) : DVSOF_OK;
        if (rc_) return rc_;
        if (x->w.need_event[id]) DVSOF_HIP_TRY(hipEventRecord(n.ev, st));
    }
    for (int l = 1; l < L; ++l) {   // `stream` continues behind every lane
        DVSOF_HIP_TRY(hipEventRecord(x->join[l - 1], lane_stream(l)));
        DVSOF_HIP_TRY(hipStreamWaitEvent(main, x->join[l - 1], 0));
    }
    if (x->trial_cur >= 0) DVSOF_HIP_TRY(hipEventRecord(x->t1, main));
    return DVSOF_OK;
}

int dvsof_exec_plan(void *exec, char *name, int name_len, int *settled)
{
    if (!exec) return DVSOF_EINVAL;
    Exec *x = (Exec *)exec;
    if (settled) *settled = x->trial_next < 0;
    copy_name(name, name_len, x->plan.name);
    return DVSOF_OK;
}

int dvsof_exec_destroy(void *exec)
{
    if (!exec) return DVSOF_EINVAL;
    destroy((Exec *)exec);
    return DVSOF_OK;
}

}  // extern "C"

// Step executor, the part that decides: everything exec.hip knows about the
// captured graph that is no HIP call.  Standard C++ only (tools/exec_sched_check.cpp
// runs it on the host under the sanitizers, tests/test_exec_schedule.py).
//
// Everything is indexed by CAPTURE ID: the position of a node in the topological
// order of the capture (topo_order).  Nodes never move; a lane plan is a launch
// order (a permutation of ids) plus a lane per id, and wire() turns a plan into
// the cross-lane waits and the events they need.
#pragma once
#include "../../include/dvsof.h"    // DVSOF_MARK_*
#include <algorithm>
#include <utility>
#include <vector>

namespace exec_sched {

enum Kind { KERNEL = 0, BUCKET = DVSOF_MARK_BUCKET, JOIN = DVSOF_MARK_JOIN, WAIT = DVSOF_MARK_WAIT, EMPTY };
inline bool is_mark(int kind) { return kind == BUCKET || kind == JOIN || kind == WAIT; }

struct Node {
    int kind = KERNEL;
    int mark_index = 0;
    float us = 1.f;             // measured duration (calibration)
    std::vector<int> deps;      // ids of the nodes this one depends on
};

// What is a fact of the capture, fixed at creation (build).
struct Sched {
    int max_lanes = 1;
    std::vector<Node> nodes;                // deps REWRITTEN: kernels bypass BUCKET marks (build)
    std::vector<std::vector<int>> succ;     // of the rewritten deps, ascending
    std::vector<int> lane0;                 // the greedy chain split
    std::vector<char> update;               // belongs on the UPDATE lane when there is one (build)
    std::vector<std::vector<int>> window;   // BUCKET mark: the kernels captured behind it that are NOT
                                            // behind its WAIT / the JOIN mark (they must not touch the bucket)
};

// A lane plan: launch order (node ids) and lane by node id.
struct Plan {
    const char *name;
    std::vector<int> order, lane;
};

struct Wiring {
    std::vector<int> pos;                   // position in the launch order, by id
    std::vector<int> lane;                  // effective lane (update lane = max_lanes)
    std::vector<std::vector<int>> wait;     // nodes of other lanes to wait for before the launch
    std::vector<char> need_event;           // another lane waits for this node
    std::vector<int> wait_for;              // WAIT: id of the BUCKET mark whose collective the lane waits for
    std::vector<char> xdone_used;           // BUCKET: a WAIT mark refers to it
    int n_lanes = 0, n_events = 0, n_waits = 0;
};

inline std::vector<std::vector<int>> successors(const std::vector<Node> &nodes)
{
    std::vector<std::vector<int>> succ(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i)
        for (int d : nodes[i].deps) succ[d].push_back((int)i);
    return succ;
}

// Topological order of n nodes under edges (from, to); ties by position in the node
// list (= capture order of a stream capture), so that the host issues kernels in
// the eager order.  order[id] = list position; deps[id] = ids, ascending.  False on
// an edge that names an unknown node and on a cycle.
inline bool topo_order(int n, const std::vector<std::pair<int, int>> &edges, std::vector<int> &order,
                       std::vector<std::vector<int>> &deps)
{
    std::vector<std::vector<int>> rdeps(n), rsucc(n);
    for (const auto &e : edges) {
        if (e.first < 0 || e.first >= n || e.second < 0 || e.second >= n) return false;
        rdeps[e.second].push_back(e.first);
        rsucc[e.first].push_back(e.second);
    }
    std::vector<int> indeg(n), ready, pos(n);
    for (int i = 0; i < n; ++i) {
        indeg[i] = (int)rdeps[i].size();
        if (!indeg[i]) ready.push_back(i);
    }
    auto cmp = [](int a, int b) { return a > b; };   // min-heap on the list position
    std::make_heap(ready.begin(), ready.end(), cmp);
    order.clear();
    while (!ready.empty()) {
        std::pop_heap(ready.begin(), ready.end(), cmp);
        const int i = ready.back();
        ready.pop_back();
        pos[i] = (int)order.size();
        order.push_back(i);
        for (int s : rsucc[i])
            if (--indeg[s] == 0) {
                ready.push_back(s);
                std::push_heap(ready.begin(), ready.end(), cmp);
            }
    }
    if ((int)order.size() != n) return false;   // cycle: not a DAG
    deps.assign(n, {});
    for (int id = 0; id < n; ++id) {
        for (int d : rdeps[order[id]]) deps[id].push_back(pos[d]);
        std::sort(deps[id].begin(), deps[id].end());
    }
    return true;
}

// nodes in capture order with their dependencies AS CAPTURED (ids below their own).
inline Sched build(std::vector<Node> nodes, int max_lanes)
{
    const int nn = (int)nodes.size();
    Sched s;
    s.max_lanes = max_lanes;
    for (auto &n : nodes) std::sort(n.deps.begin(), n.deps.end());
    // lane: extend the chain of a dependency that is still the tail of its
    // lane (lowest lane first); else open a lane; else share the last one
    s.lane0.resize(nn);
    std::vector<int> tail;
    for (int i = 0; i < nn; ++i) {
        int lane = -1;
        for (int d : nodes[i].deps) {
            const int l = s.lane0[d];
            if (tail[l] == d && (lane < 0 || l < lane)) lane = l;
        }
        if (lane < 0) {
            if ((int)tail.size() < max_lanes) {
                lane = (int)tail.size();
                tail.push_back(-1);
            } else {
                lane = max_lanes - 1;
            }
        }
        s.lane0[i] = lane;
        tail[lane] = i;
    }
    // The exchange window of every BUCKET mark, from the dependencies AS CAPTURED: the kernels
    // that follow the mark in the capture but neither its WAIT mark nor (without one) the JOIN
    // mark.  The rewrite below lets exactly these run beside the collective, which is only
    // right when none of them reads or writes the bucket -- dvsof_exec_mark_window hands the
    // set to the caller, who knows the kernels' argument layouts (capture.py refuses the
    // recording when one of them carries a pointer into the bucket).
    {
        const std::vector<std::vector<int>> succ = successors(nodes);
        auto reach = [&](int from, std::vector<char> &seen) {
            std::vector<int> todo{from};
            seen[from] = 1;
            while (!todo.empty()) {
                const int v = todo.back();
                todo.pop_back();
                for (int s_ : succ[v])
                    if (!seen[s_]) {
                        seen[s_] = 1;
                        todo.push_back(s_);
                    }
            }
        };
        s.window.resize(nn);
        for (int m = 0; m < nn; ++m) {
            if (nodes[m].kind != BUCKET) continue;
            std::vector<char> behind(nn, 0), safe(nn, 0);
            reach(m, behind);
            bool has_wait = false;
            for (int j = 0; j < nn; ++j)
                if (nodes[j].kind == WAIT && nodes[j].mark_index == nodes[m].mark_index) {
                    has_wait = true;
                    reach(j, safe);
                }
            if (!has_wait)
                for (int j = 0; j < nn; ++j)
                    if (nodes[j].kind == JOIN && behind[j]) reach(j, safe);
            for (int j = 0; j < nn; ++j)
                if (j != m && behind[j] && !safe[j] && nodes[j].kind == KERNEL) s.window[m].push_back(j);
        }
    }
    // A BUCKET mark is a side effect of its stream, not a producer: what follows it in the
    // capture follows what PRECEDED it.  Kernels inherit the mark's dependencies instead of
    // depending on the mark (else the kernel behind a mark is tied to the mark's lane and, in
    // another lane, pays a cross-lane wait per bucket); the other marks keep theirs (the JOIN
    // has to be issued behind every collective, a WAIT behind its own).
    for (int i = 0; i < nn; ++i) {      // (ascending: the dependencies of a mark are never rewritten)
        if (is_mark(nodes[i].kind)) continue;
        std::vector<int> out, todo = nodes[i].deps;
        while (!todo.empty()) {
            const int d = todo.back();
            todo.pop_back();
            if (nodes[d].kind == BUCKET)
                todo.insert(todo.end(), nodes[d].deps.begin(), nodes[d].deps.end());
            else if (std::find(out.begin(), out.end(), d) == out.end())
                out.push_back(d);
        }
        std::sort(out.begin(), out.end());
        nodes[i].deps = out;
    }
    s.succ = successors(nodes);
    // Nodes of the update lane: a kernel whose every dependency is a WAIT mark or such a kernel
    // (parallel.GradReducer captures a bucket's optimizer update on the exchange stream, behind the
    // bucket's WAIT mark: the update follows the collective in stream order and no compute lane waits
    // for either), and the WAIT marks all of whose successors are such kernels.
    s.update.assign(nn, 0);
    for (int i = 0; i < nn; ++i) {      // capture order is a topological order
        if (nodes[i].kind != KERNEL || nodes[i].deps.empty()) continue;
        bool all = true;
        for (int d : nodes[i].deps)
            if (!(nodes[d].kind == WAIT || s.update[d])) all = false;
        s.update[i] = all;
    }
    for (int k = nn; k-- > 0;) {        // (descending: a WAIT mark's successor may be the next WAIT mark
                                        // of the branch -- an update that collects several buckets)
        if (nodes[k].kind != WAIT || s.succ[k].empty()) continue;
        bool all = true;
        for (int s_ : s.succ[k])
            if (!(s.update[s_] || nodes[s_].kind == JOIN)) all = false;
        s.update[k] = all;
    }
    s.nodes = std::move(nodes);
    return s;
}

inline Plan identity_plan(const char *name, int nn)
{
    Plan p{name, std::vector<int>(nn), std::vector<int>(nn, 0)};
    for (int id = 0; id < nn; ++id) p.order[id] = id;
    return p;
}

// Plan "chain": the greedy chain split of build, capture order.
inline Plan plan_chain(const Sched &s)
{
    Plan p = identity_plan("chain", (int)s.nodes.size());
    p.lane = s.lane0;
    return p;
}

// Plan "paths", lanes by measured time: lane l = the longest path (sum of node
// durations) through the nodes no earlier lane took; the last lane takes the
// rest.  Launch order = capture order.
inline Plan plan_paths(const Sched &s)
{
    const int nn = (int)s.nodes.size();
    Plan p = identity_plan("paths", nn);
    std::vector<char> taken(nn, 0);
    int left = nn;
    for (int i = 0; i < nn; ++i)    // the update lane's nodes take no compute lane (wire() places them)
        if (s.update[i]) {
            taken[i] = 1;
            p.lane[i] = s.max_lanes - 1;
            --left;
        }
    for (int l = 0; l < s.max_lanes && left > 0; ++l) {
        if (l == s.max_lanes - 1) {
            for (int i = 0; i < nn; ++i)
                if (!taken[i]) p.lane[i] = l;
            break;
        }
        std::vector<double> best(nn, 0.0);
        std::vector<int> from(nn, -1);
        int end = -1;
        for (int i = 0; i < nn; ++i) {
            if (taken[i]) continue;
            double b = 0.0;
            for (int d : s.nodes[i].deps)
                if (!taken[d] && best[d] > b) {
                    b = best[d];
                    from[i] = d;
                }
            best[i] = b + (double)s.nodes[i].us;
            if (end < 0 || best[i] > best[end]) end = i;
        }
        for (int i = end; i >= 0; i = from[i]) {
            p.lane[i] = l;
            taken[i] = 1;
            --left;
        }
    }
    return p;
}

// Plan "list", list scheduling on the measured durations: lanes are in-order
// queues; of the nodes whose dependencies are placed the one with the longest
// remaining path to the end of the step goes next, onto the lane where it can
// start first (a dependency in another lane costs `hop` us on top of its end).
// The chain that bounds the step keeps flowing on one lane; whatever hangs off
// it (weight gradients, folds, prepared forms) fills the other.  Also fixes
// the LAUNCH order: the order nodes were placed in.
// Equal priorities go by capture id.  (Before the scheduler was written in ids they
// went by the position in the launch order in effect, which is the capture id where
// the plans are made: at the one calibration of an executor, before any plan.)
inline Plan plan_list(const Sched &s, double hop)
{
    const int nn = (int)s.nodes.size(), L = s.max_lanes;
    std::vector<std::vector<int>> succ = s.succ;
    std::vector<int> indeg(nn, 0);
    for (int i = 0; i < nn; ++i) indeg[i] = (int)s.nodes[i].deps.size();
    // marks keep their capture order: every rank issues the same collectives in the
    // same order whatever its own measured durations say
    for (int i = 0, last = -1; i < nn; ++i)
        if (is_mark(s.nodes[i].kind)) {
            if (last >= 0) {
                succ[last].push_back(i);
                ++indeg[i];
            }
            last = i;
        }
    std::vector<double> bl(nn, 0.0);
    for (int i = nn - 1; i >= 0; --i) {     // ids are a topological order
        double b = 0.0;
        for (int s_ : succ[i]) b = std::max(b, bl[s_]);
        bl[i] = b + (double)s.nodes[i].us;
    }
    std::vector<double> fin(nn, 0.0), free_at(L, 0.0);
    std::vector<int> ready;
    for (int i = 0; i < nn; ++i)
        if (!indeg[i]) ready.push_back(i);
    Plan p{"list", {}, std::vector<int>(nn, 0)};
    p.order.reserve(nn);
    while (!ready.empty()) {
        size_t pick = 0;
        for (size_t k = 1; k < ready.size(); ++k) {
            const int a = ready[k], b = ready[pick];
            if (bl[a] > bl[b] || (bl[a] == bl[b] && a < b)) pick = k;
        }
        const int i = ready[pick];
        ready.erase(ready.begin() + (long)pick);
        int best_l = L - 1;
        double best_t = 0.0;
        if (s.update[i]) {      // on the update lane: occupies no compute lane
            for (int d : s.nodes[i].deps) best_t = std::max(best_t, fin[d]);
        } else {
            for (int l = 0; l < L; ++l) {
                double t = free_at[l];
                for (int d : s.nodes[i].deps) t = std::max(t, fin[d] + (p.lane[d] != l ? hop : 0.0));
                if (l == 0 || t < best_t) {
                    best_t = t;
                    best_l = l;
                }
            }
        }
        p.lane[i] = best_l;
        fin[i] = best_t + (double)s.nodes[i].us;
        if (!s.update[i]) free_at[best_l] = fin[i];
        p.order.push_back(i);
        for (int s_ : succ[i])
            if (--indeg[s_] == 0) ready.push_back(s_);
    }
    return p;
}

// From lanes to waits and events: a node waits for its dependencies in other
// lanes, minus those an earlier wait of its lane on the same producer lane
// already covers (lanes run in order: waiting for node d covers d's
// predecessors in its lane).  The update lane is one more lane (index
// max_lanes) for the nodes that belong on it.  Creates nothing: says what is needed.
inline Wiring wire(const Sched &s, const Plan &p, bool update_lane_active)
{
    const int nn = (int)s.nodes.size();
    Wiring w;
    w.pos.resize(nn);
    w.lane.resize(nn);
    w.wait.resize(nn);
    w.need_event.assign(nn, 0);
    w.wait_for.assign(nn, -1);
    w.xdone_used.assign(nn, 0);
    for (int k = 0; k < nn; ++k) w.pos[p.order[k]] = k;
    for (int i = 0; i < nn; ++i) {
        w.lane[i] = (s.update[i] && update_lane_active) ? s.max_lanes : p.lane[i];
        w.n_lanes = std::max(w.n_lanes, w.lane[i] + 1);
    }
    for (int i = 0; i < nn; ++i) {      // WAIT marks find their BUCKET mark (same mark index)
        if (s.nodes[i].kind != WAIT) continue;
        for (int j = 0; j < nn; ++j)
            if (s.nodes[j].kind == BUCKET && s.nodes[j].mark_index == s.nodes[i].mark_index) {
                w.wait_for[i] = j;
                w.xdone_used[j] = 1;
            }
    }
    std::vector<std::vector<int>> seen(w.n_lanes, std::vector<int>(w.n_lanes, -1));
    for (int i : p.order) {
        std::vector<int> c;     // positions of the dependencies in other lanes, the latest first
        for (int d : s.nodes[i].deps)
            if (w.lane[d] != w.lane[i]) c.push_back(w.pos[d]);
        std::sort(c.begin(), c.end());
        for (auto k = c.rbegin(); k != c.rend(); ++k) {
            const int d = p.order[*k];
            int &covered = seen[w.lane[i]][w.lane[d]];
            if (covered >= *k) continue;
            covered = *k;
            w.wait[i].push_back(d);
            w.n_events += !w.need_event[d];
            w.need_event[d] = 1;
        }
        w.n_waits += (int)w.wait[i].size();
    }
    return w;
}

}  // namespace exec_sched

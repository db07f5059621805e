// Stand-alone host program for the step executor's scheduler (csrc/exec_sched.h): fixed
// captures whose expected lanes, waits, windows and plans are derived by hand from the rules
// (the derivation stands next to each expectation), and seeded random captures on which a
// validator written from the definition of happens-before checks every plan and both states
// of the update lane.  It makes no HIP call and needs no GPU; build it with the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/exec_sched_check.cpp -o exec_sched_check
// One line per case; exit status 1 on any mismatch (tests/test_exec_schedule.py).
#include "../dvs_of_training_framework_amd/csrc/exec_sched.h"
#include <stdint.h>
#include <stdio.h>
#include <string>

using namespace exec_sched;
typedef std::vector<int> V;
typedef std::vector<V> VV;

static int bad = 0;
static long checks = 0;

static bool check(bool ok, const char *what)
{
    ++checks;
    if (!ok) {
        ++bad;
        printf("  BAD: %s\n", what);
    }
    return ok;
}

static Node node(int kind, V deps, int mark_index = 0, float us = 1.f)
{
    Node n;
    n.kind = kind;
    n.mark_index = mark_index;
    n.us = us;
    n.deps = deps;
    return n;
}
static Node K(V deps, float us = 1.f) { return node(KERNEL, deps, 0, us); }

// "1 3" -> {1, 3}
static V v(const char *s)
{
    V out;
    bool in_number = false;
    for (; *s; ++s) {
        const bool digit = *s >= '0' && *s <= '9';
        if (digit && in_number) out.back() = 10 * out.back() + *s - '0';
        else if (digit) out.push_back(*s - '0');
        in_number = digit;
    }
    return out;
}

// ";2 4;;4" -> {{}, {2, 4}, {}, {4}}: one list per node
static VV vv(const char *s)
{
    VV out(1);
    std::string item;
    for (;; ++s) {
        if (*s == ';' || !*s) {
            out.back() = v(item.c_str());
            item.clear();
            if (!*s) return out;
            out.push_back({});
        } else {
            item += *s;
        }
    }
}

// A capture written as "kind deps; ...", one node per id: K kernel, E empty, B<i> BUCKET mark of
// index i, W<i> its WAIT mark, J the JOIN mark.  "K; B0 0; K 1": kernel 0, BUCKET#0 behind it, ...
static std::vector<Node> graph(const char *s)
{
    std::vector<Node> g;
    std::string item;
    for (;; ++s) {
        if (*s != ';' && *s) {
            item += *s;
            continue;
        }
        const size_t at = item.find_first_not_of(' ');
        const char k = item[at];
        const bool indexed = k == 'B' || k == 'W';
        g.push_back(node(k == 'K' ? KERNEL : k == 'E' ? EMPTY : k == 'B' ? BUCKET : k == 'W' ? WAIT : JOIN,
                         v(item.c_str() + at + (indexed ? 2 : 1)), indexed ? item[at + 1] - '0' : 0));
        item.clear();
        if (!*s) return g;
    }
}

static V flagged(const std::vector<char> &f)
{
    V out;
    for (size_t i = 0; i < f.size(); ++i)
        if (f[i]) out.push_back((int)i);
    return out;
}

static void done(const char *name, int bad0) { printf("%s case %s\n", bad == bad0 ? "ok " : "BAD", name); }

// ------------------------------------------------------------------ fixed cases
static void case_a()
{
    const int bad0 = bad;
    const Sched s = build(graph("K; K 0; K 0; K 1; K 2; K 3 4; K 1 3"), 2);
    // 0 opens lane 0; 1 extends it (0 is its tail); 2: 0 is no tail any more, a lane is free: lane 1;
    // 3 extends lane 0 behind 1, 4 lane 1 behind 2; 5: 3 and 4 are both tails, the lowest lane: 0;
    // 6: neither 1 nor 3 is a tail (5 and 4 are) and both lanes exist: the last lane, 1
    check(s.lane0 == v("0 0 1 0 1 0 1"), "A: chain lanes");
    const Plan p = plan_chain(s);
    check(p.order == v("0 1 2 3 4 5 6") && p.lane == s.lane0, "A: chain plan = capture order, greedy lanes");
    const Wiring w = wire(s, p, false);
    // 2 (lane 1) needs 0 (lane 0); 5 (lane 0) needs 4 (lane 1), 3 is its own lane; 6 (lane 1) needs 3 and
    // 1 of lane 0, descending: 3 first (lane 1 has waited for position 0 so far), which covers 1
    check(w.wait == vv(";;0;;;4;3"), "A: waits");
    check(flagged(w.need_event) == v("0 3 4"), "A: events");
    check(w.n_waits == 3 && w.n_events == 3 && w.n_lanes == 2, "A: counts");
    check(w.lane == s.lane0 && w.pos == p.order, "A: lanes and positions");
    done("A split and wait elimination", bad0);
}

static std::vector<Node> graph_b() { return graph("K; B0 0; K 1; B1 2; K 3; J 4; K 5"); }

static void case_b()
{
    const int bad0 = bad;
    const Sched s = build(graph_b(), 2);
    VV deps;
    for (const Node &n : s.nodes) deps.push_back(n.deps);
    // kernels see through BUCKET marks: 2 takes 1's {0}, 4 takes 3's {2}; marks (1, 3, 5) keep theirs;
    // 6 follows a JOIN, which is no BUCKET
    check(deps == vv(";0;0;2;2;4;5"), "B: rewritten dependencies");
    // no WAIT mark: safe = behind the JOIN (5) = {5, 6}.  Behind #0 (node 1): 2..6, kernels 2, 4, 6,
    // minus safe: {2, 4}.  Behind #1 (node 3): 4, 5, 6: {4}
    check(s.window == vv(";2 4;;4;;;"), "B: windows");
    check(flagged(s.update).empty(), "B: no update lane");
    // as captured every node follows the one before, the tail of lane 0
    check(s.lane0 == V(7, 0), "B: one chain");
    const Wiring w = wire(s, plan_chain(s), true);
    check(w.n_lanes == 1 && w.n_waits == 0 && w.n_events == 0 && flagged(w.xdone_used).empty(), "B: wiring");
    done("B bypass and windows without WAIT", bad0);
}

static std::vector<Node> graph_c() { return graph("K; B0 0; K 1; W0 1; K 3; K 4; B1 2; W1 5 6; K 7; J 2 8; K 9"); }

static void case_c()
{
    const int bad0 = bad;
    const Sched s = build(graph_c(), 2);
    // 4 follows only WAIT 3, 5 only 4, 8 only WAIT 7: update kernels.  2 follows (through BUCKET 1) kernel
    // 0, 10 follows a JOIN: not.  WAIT 7's successors: {8}; WAIT 3's: {4}: both on the lane
    check(flagged(s.update) == v("3 4 5 7 8"), "C: update lane");
    // behind #0 (node 1): 2..10; safe = behind WAIT 3 = {3,4,5,7,8,9,10}: kernel 2 is left.
    // behind #1 (node 6): 7..10, all behind WAIT 7
    check(s.window[1] == v("2") && s.window[6].empty(), "C: windows");
    // as captured: 0,1,2 chain on lane 0; 3 follows 1, no tail: lane 1, 4 and 5 behind it; 6 extends
    // lane 0 behind 2; 7: 5 (lane 1) and 6 (lane 0) are tails: lane 0; 8, 9 (behind 8), 10 extend it
    check(s.lane0 == v("0 0 0 1 1 1 0 0 0 0 0"), "C: chain lanes");
    const Plan p = plan_chain(s);
    const Wiring on = wire(s, p, true), off = wire(s, p, false);
    check(on.wait_for[3] == 1 && on.wait_for[7] == 6 && off.wait_for[3] == 1 && off.wait_for[7] == 6, "C: wait_for");
    check(flagged(on.xdone_used) == v("1 6") && flagged(off.xdone_used) == v("1 6"), "C: xdone_used");
    check(on.lane == v("0 0 0 2 2 2 0 2 2 0 0") && on.n_lanes == 3, "C: update lane active");
    check(off.lane == s.lane0 && off.n_lanes == 2, "C: update lane inactive");
    // rewritten: 2:{0} 3:{1} 4:{3} 5:{4} 6:{2} 7:{5,6} 8:{7} 9:{2,8} 10:{9}.  Active: 3 waits for 1
    // (lane 0), 7 for 6 (lane 0, later than 1), 9 (lane 0) for 8 (lane 2)
    check(on.wait == vv(";;;1;;;;6;;8;") && flagged(on.need_event) == v("1 6 8"), "C: waits, active");
    // inactive: 3 (lane 1) waits for 1, 7 (lane 0) for 5 (lane 1); 8, 9, 10 follow on lane 0
    check(off.wait == vv(";;;1;;;;5;;;") && flagged(off.need_event) == v("1 5"), "C: waits, inactive");
    done("C WAIT marks and the update lane", bad0);
}

static void case_d()
{
    const int bad0 = bad;
    std::vector<Node> g = graph_c();
    const float us[] = {1, 0, 100, 0, 1, 1, 50, 0, 1, 0, 1};   // 2, in front of BUCKET#1, and that mark are long
    for (int i = 0; i < 11; ++i) g[i].us = us[i];
    const Plan p = plan_list(build(g, 2), 8.0);
    // edges: the rewritten ones of case C plus the mark chain 1>3>6>7>9.  Remaining path: 10:1 9:1 8:2 7:2
    // 6:52 5:3 4:4 3:max(4,52) 2:100+52 1:52 0:153.  0; of {1,2}: 2; 6 still waits for mark 3 (WITHOUT the
    // chain it would go here, in front of 1: 52 against 4); 1; 3; of {4,6}: 6; 4; 5; 7; 8; 9; 10
    check(p.order == v("0 2 1 3 6 4 5 7 8 9 10"), "D: launch order");
    // lanes (hop 8): 0 and 2 on lane 0 (ends 1, 101); 1: lane 0 is free at 101, lane 1 at 1+8; the update
    // nodes 3,4,5,7,8 take no compute lane (written as the last), ends 9,10,11,151,152; 6: lane 0 at 101
    // against 101+8; 9: lane 0 at 152+8 against lane 1 at max(101+8,152); 10: lane 1 at 152 against 160
    check(p.lane == v("0 1 0 1 1 1 0 1 1 1 1"), "D: lanes");
    V marks;
    for (int id : p.order)
        if (is_mark(g[id].kind)) marks.push_back(id);
    check(marks == v("1 3 6 7 9"), "D: marks in capture order");
    done("D plan_list keeps collectives in capture order", bad0);
}

static void case_e()
{
    const int bad0 = bad;
    // 0 > 1 > 2 (10 us each) and 0 > 3 > 4 (3 us each) meet in 5; 6 hangs off 0
    std::vector<Node> g = graph("K; K 0; K 1; K 0; K 3; K 2 4; K 0");
    const float us[] = {1, 10, 10, 3, 3, 1, 1};
    for (int i = 0; i < 7; ++i) g[i].us = us[i];
    // longest path: 0 (1) 1 (11) 2 (21) 5 (22): lane 0; the rest on the last lane
    const Plan p = plan_paths(build(g, 2));
    check(p.order == v("0 1 2 3 4 5 6") && p.lane == v("0 0 0 1 1 0 1"), "E: two lanes");
    // three lanes: lane 1 = the longest path through what is left, 3 (3) 4 (6); 6 on the last
    check(plan_paths(build(g, 3)).lane == v("0 0 0 1 1 0 2"), "E: three lanes");
    check(plan_paths(build(g, 1)).lane == V(7, 0), "E: one lane");
    done("E plan_paths", bad0);
}

static void case_f()
{
    const int bad0 = bad;
    V order;
    VV deps;
    check(!topo_order(3, {{0, 1}, {1, 2}, {2, 1}}, order, deps), "F: cycle");
    check(!topo_order(3, {{0, 5}}, order, deps) && !topo_order(3, {{-1, 1}}, order, deps), "F: unknown node");
    // 1 and 3 are free: 1 first (list position), which frees 2; then 2, 3, and 0 behind 3
    check(topo_order(4, {{3, 0}, {1, 2}}, order, deps) && order == v("1 2 3 0") && deps == vv(";0;;2"),
          "F: ties by list position");
    done("F refusals", bad0);
}

// ------------------------------------------------------------------ seeded captures
static uint64_t lcg_state = 0x9e3779b97f4a7c15ull;
static int rnd(int n)      // 0 .. n-1
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((lcg_state >> 33) % (uint64_t)n);
}

// A DAG over shuffled labels, ordered by topo_order (which is checked on the way).
static std::vector<Node> random_dag(int n)
{
    V label(n);     // label[k] = list position of the k-th node of a hidden topological order
    for (int i = 0; i < n; ++i) label[i] = i;
    for (int i = n - 1; i > 0; --i) std::swap(label[i], label[rnd(i + 1)]);
    std::vector<std::pair<int, int>> edges;
    for (int k = 1; k < n; ++k)
        for (int e = rnd(4); e > 0; --e) edges.push_back({label[rnd(k)], label[k]});
    V order;
    VV deps;
    check(topo_order(n, edges, order, deps), "topo_order accepts a DAG");
    // the definition: of the nodes whose predecessors are all placed, the lowest list position
    std::vector<char> placed(n, 0);
    for (int k = 0; k < n; ++k) {
        int want = -1;
        for (int v = 0; v < n && want < 0; ++v) {
            bool free_ = !placed[v];
            for (const auto &e : edges)
                if (e.second == v && !placed[e.first]) free_ = false;
            if (free_) want = v;
        }
        check(order[k] == want, "topo_order: ties by list position");
        placed[order[k]] = 1;
    }
    std::vector<Node> g(n);
    for (int i = 0; i < n; ++i) {
        g[i] = node(rnd(10) ? KERNEL : EMPTY, deps[i], 0, 0.5f + (float)rnd(200));
        for (const auto &e : edges)
            if (e.second == order[i]) check(std::count(order.begin(), order.begin() + i, e.first) == 1, "dep precedes");
    }
    return g;
}

// A captured data-parallel step in the shape of cases B and C: a compute chain with BUCKET marks
// in it, weight-gradient style kernels hanging off it, per bucket (with_wait) a WAIT mark and
// update kernels on a branch of their own, a JOIN mark and the kernels behind it.
static std::vector<Node> random_step(int n, bool with_wait)
{
    std::vector<Node> g;
    int main_tail = -1, branch_tail = -1, bucket = 0;
    V kernels;
    auto us = [] { return 0.5f + (float)rnd(100); };
    while ((int)g.size() < n - 3) {
        const int r = rnd(6);
        if (r == 0 && main_tail >= 0) {
            const int b = (int)g.size();
            g.push_back(node(BUCKET, {main_tail}, bucket, 0.f));
            main_tail = b;
            if (with_wait && rnd(4)) {      // (some buckets are left to the JOIN mark)
                V d{b};
                if (branch_tail >= 0) d.push_back(branch_tail);
                g.push_back(node(WAIT, d, bucket, 0.f));
                branch_tail = (int)g.size() - 1;
                for (int u = rnd(3); u > 0 && (int)g.size() < n - 3; --u) {
                    g.push_back(K({branch_tail}, us()));
                    branch_tail = (int)g.size() - 1;
                }
            }
            ++bucket;
        } else if (r == 1 && !kernels.empty()) {    // off the chain
            V d{kernels[rnd((int)kernels.size())]};
            if (rnd(2)) d.push_back(kernels[rnd((int)kernels.size())]);
            g.push_back(K(d, us()));
            kernels.push_back((int)g.size() - 1);
        } else {
            V d;
            if (main_tail >= 0) d.push_back(main_tail);
            if (!kernels.empty() && rnd(3) == 0) d.push_back(kernels[rnd((int)kernels.size())]);
            g.push_back(K(d, us()));
            main_tail = (int)g.size() - 1;
            kernels.push_back(main_tail);
        }
    }
    V d{main_tail};
    if (branch_tail >= 0) d.push_back(branch_tail);
    g.push_back(node(JOIN, d, 0, 0.f));
    g.push_back(K({(int)g.size() - 1}, us()));
    g.push_back(K({(int)g.size() - 1}, us()));
    return g;
}

// ancestors as bit sets (at most 40 nodes); ids are a topological order
static std::vector<uint64_t> ancestors(const std::vector<Node> &g)
{
    std::vector<uint64_t> anc(g.size(), 0);
    for (size_t v = 0; v < g.size(); ++v)
        for (int d : g[v].deps) anc[v] |= anc[d] | (1ull << d);
    return anc;
}

// what a kernel follows once BUCKET marks are looked through (the definition, recursively)
static void through_buckets(const std::vector<Node> &g, int v, uint64_t &out)
{
    for (int d : g[v].deps)
        if (g[d].kind == BUCKET) through_buckets(g, d, out);
        else out |= 1ull << d;
}

static void validate_sched(const std::vector<Node> &g, const Sched &s)
{
    const int n = (int)g.size();
    const std::vector<uint64_t> anc = ancestors(g);
    for (int v = 0; v < n; ++v) {
        uint64_t want = 0, got = 0;
        if (is_mark(g[v].kind))
            for (int d : g[v].deps) want |= 1ull << d;
        else
            through_buckets(g, v, want);
        for (int d : s.nodes[v].deps) got |= 1ull << d;
        check(want == got, "rewritten dependencies");
        check(s.lane0[v] >= 0 && s.lane0[v] < s.max_lanes, "greedy lane in range");
    }
    for (int m = 0; m < n; ++m) {       // 5. windows, as captured
        if (g[m].kind != BUCKET) {
            check(s.window[m].empty(), "window of a non-BUCKET node");
            continue;
        }
        uint64_t guards = 0, joins = 0, got = 0, want = 0;
        for (int j = 0; j < n; ++j) {
            if (g[j].kind == WAIT && g[j].mark_index == g[m].mark_index) guards |= 1ull << j;
            if (g[j].kind == JOIN && (anc[j] >> m & 1)) joins |= 1ull << j;
        }
        if (!guards) guards = joins;
        for (int j : s.window[m]) {
            got |= 1ull << j;
            check(g[j].kind == KERNEL && (anc[j] >> m & 1), "window member is a kernel behind the mark");
            check(!(anc[j] & guards), "window member is not behind the bucket's WAIT / JOIN");
        }
        for (int j = 0; j < n; ++j)     // and nothing is missing: the audit reads exactly these
            if (g[j].kind == KERNEL && (anc[j] >> m & 1) && !(anc[j] & guards)) want |= 1ull << j;
        check(got == want, "window is complete");
    }
}

static void validate_plan(const std::vector<Node> &g, const Sched &s, const Plan &p, bool active)
{
    const int n = (int)g.size();
    const Wiring w = wire(s, p, active);
    V pos(n, -1);
    bool perm = (int)p.order.size() == n && (int)p.lane.size() == n;
    for (int k = 0; perm && k < n; ++k) {
        const int id = p.order[k];
        perm = id >= 0 && id < n && pos[id] < 0;
        if (perm) pos[id] = k;
    }
    if (!check(perm, "1. order is a permutation")) return;
    int last_mark = -1, lanes = 0, waits = 0;
    std::vector<char> waited(n, 0);
    // happens-before, by launch position: hb[v] = everything that has ended when v starts
    std::vector<uint64_t> hb(n, 0);
    std::vector<int> lane_tail(s.max_lanes + 1, -1);
    for (int id : p.order) {
        const int l = w.lane[id];
        check(l == (active && s.update[id] ? s.max_lanes : p.lane[id]) && p.lane[id] >= 0 && p.lane[id] < s.max_lanes,
              "effective lane");
        lanes = std::max(lanes, l + 1);
        if (lane_tail[l] >= 0) hb[id] |= hb[lane_tail[l]] | (1ull << lane_tail[l]);   // same lane, earlier in order
        lane_tail[l] = id;
        for (int d : w.wait[id]) {      // an emitted wait: d's event is recorded before this launch
            check(pos[d] < pos[id], "a wait refers to an earlier launch");
            hb[id] |= hb[d] | (1ull << d);
            waited[d] = 1;
            ++waits;
        }
        for (int d : s.nodes[id].deps) {
            check(pos[d] < pos[id], "1. order is topological");
            check(hb[id] >> d & 1, "2. dependency enforced");
        }
        if (is_mark(g[id].kind)) {
            check(id > last_mark, "4. marks in capture order");
            last_mark = id;
        }
    }
    int events = 0;
    for (int v = 0; v < n; ++v) {
        check((bool)w.need_event[v] == (bool)waited[v], "3. events exactly on the waited-for nodes");
        events += waited[v];
    }
    check(w.n_lanes == lanes && w.n_waits == waits && w.n_events == events && w.pos == pos, "counts and positions");
}

static void property_cases()
{
    const int bad0 = bad;
    const long checks0 = checks;
    int graphs = 0;
    for (int k = 0; k < 240; ++k) {
        const int n = 5 + rnd(36), max_lanes = 1 + k % 3, family = k / 3 % 3;
        const std::vector<Node> g = family == 0 ? random_dag(n) : random_step(n, family == 2);
        const Sched s = build(g, max_lanes);
        validate_sched(g, s);
        const Plan plans[] = {plan_chain(s), plan_paths(s), plan_list(s, 8.0)};
        for (const Plan &p : plans)
            for (int active = 0; active < 2; ++active) validate_plan(g, s, p, active);
        check(plans[0].order == plans[1].order && plans[0].lane == s.lane0, "chain and paths launch in capture order");
        ++graphs;
    }
    printf("%s property cases: %d graphs, %ld checks\n", bad == bad0 ? "ok " : "BAD", graphs, checks - checks0);
}

int main()
{
    case_a();
    case_b();
    case_c();
    case_d();
    case_e();
    case_f();
    property_cases();
    printf("%d bad\n", bad);
    return bad != 0;
}

// The order plan of mldsa_vfy_verify (fips204_amd/vfy/vfy_parts.h, order_plan) on its own: pure host code, compiled with
// -fsanitize=address,undefined and run as a child process by tests/test_vfy_order_cpu.py.  enqueue() issues one runtime call per step of
// the plan, so what this program derives from the plan is what the device is told.
// The model: a lane (the caller's stream, the library's two) is a FIFO, so a step is ordered behind the step enqueued before it on its
// lane; a wait is ordered behind the latest record of its event enqueued before it (events are reused from call to call, as the
// library's pool hands them out).  Happens-before is the transitive closure.  For calls of 1, 2, 3 and 7 parts, alone and as two calls
// back to back on the same lanes and events (all 16 pairs), it asserts
//   - every step of a call follows the call's fork, and precedes the end of the caller's lane (so the call is a fork/join region);
//   - expand_a(p) and front(p) precede verify_main(p), verify_main(p) precedes ctilde(p) and expand_a(p + 2), the ring half;
//   - every stage of the first call precedes every stage of the second: they share one scratch;
//   - one part: expand_a, verify_main and ctilde on the caller's lane, nothing on ea, and the caller's lane waits for the front only;
//   - the steps of one part and of several parts are the lists written out below, step for step;
// and that the checker objects to the plan with any single record or wait deleted: a deletion it accepts would be an event that orders
// nothing.  Exit status 0 and "vfy_order OK".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fips204_amd/vfy/vfy_parts.h"

using namespace mldsa_vfy;

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

static const size_t NONE = (size_t)-1;

struct Node {
    Step st;
    size_t call;
    bool end;  // the marker behind the last step of the call on the caller's lane
};

// the steps of the calls in enqueue order, step `del_step` of call `del_call` left out
static std::vector<Node> sequence(const std::vector<OrderPlan>& calls, size_t del_call = NONE, size_t del_step = NONE) {
    std::vector<Node> seq;
    for (size_t c = 0; c < calls.size(); c++) {
        for (size_t i = 0; i < calls[c].steps.size(); i++)
            if (!(c == del_call && i == del_step)) seq.push_back(Node{calls[c].steps[i], c, false});
        seq.push_back(Node{Step{LANE_CALLER, ACT_LAUNCH, N_STAGES, 0, "end"}, c, true});
    }
    return seq;
}

// Objections to the sequence as the enqueue of calls of n_parts[c] parts; `say` prints them.
static int objections(const std::vector<Node>& seq, const std::vector<size_t>& n_parts, bool say) {
    int bad = 0;
    auto object = [&](const std::string& what) {
        if (say) std::fprintf(stderr, "  objection: %s\n", what.c_str());
        bad++;
    };
    const size_t n = seq.size();
    // ---- happens-before: every edge points forward in enqueue order, so one pass in that order closes it
    std::vector<std::vector<char>> before(n, std::vector<char>(n, 0));  // before[j][i]: i precedes j
    size_t last_on[N_LANES] = {NONE, NONE, NONE};
    std::vector<size_t> latest_record, waits_of(n, 0);
    auto edge = [&](size_t i, size_t j) {
        for (size_t k = 0; k < n; k++) before[j][k] |= before[i][k];
        before[j][i] = 1;
    };
    for (size_t j = 0; j < n; j++) {
        const Step& st = seq[j].st;
        if (last_on[st.lane] != NONE) edge(last_on[st.lane], j);
        last_on[st.lane] = j;
        if (seq[j].end || st.act == ACT_LAUNCH) continue;
        if (latest_record.size() <= st.n) latest_record.resize(st.n + 1, NONE);
        if (st.act == ACT_RECORD) {
            latest_record[st.n] = j;
        } else {
            const size_t r = latest_record[st.n];
            if (r == NONE) {
                object("a wait for an event that was never recorded");  // (the runtime lets such a wait through)
            } else {
                if (seq[r].call != seq[j].call) object("a wait bound to another call's record");
                if (seq[r].st.lane == st.lane) object("a wait for an event of its own lane");
                edge(r, j);
                waits_of[r]++;
            }
        }
    }
    for (size_t j = 0; j < n; j++)
        if (!seq[j].end && seq[j].st.act == ACT_RECORD && waits_of[j] == 0) object("a record nobody waits for");
    auto precedes = [&](size_t i, size_t j) { return i != NONE && j != NONE && before[j][i]; };

    // ---- per call
    std::vector<std::vector<size_t>> stages_of(n_parts.size());  // [call][part * N_STAGES + stage] -> node
    for (size_t c = 0; c < n_parts.size(); c++) {
        std::vector<size_t>& at = stages_of[c];
        at.assign(n_parts[c] * N_STAGES, NONE);
        size_t fork = NONE, end = NONE;
        for (size_t j = 0; j < n; j++) {
            if (seq[j].call != c) continue;
            if (fork == NONE) fork = j;
            if (seq[j].end) end = j;
            if (seq[j].end || seq[j].st.act != ACT_LAUNCH) continue;
            const size_t slot = seq[j].st.n * N_STAGES + seq[j].st.stage;
            if (seq[j].st.n >= n_parts[c] || at[slot] != NONE) object("a stage launched twice or for a part the call does not have");
            else at[slot] = j;
        }
        if (fork == NONE || seq[fork].st.act != ACT_RECORD || seq[fork].st.lane != LANE_CALLER) {
            object("the call does not open with a record on the caller's lane");
            continue;
        }
        for (size_t j = 0; j < n; j++) {
            if (seq[j].call != c || j == fork) continue;
            if (!precedes(fork, j)) object("a step that does not follow the fork");
            if (j != end && !precedes(j, end)) object("a step that does not precede the end of the caller's lane");
        }
        for (size_t p = 0; p < n_parts[c]; p++) {
            const size_t ea = at[p * N_STAGES + STAGE_EXPAND_A], fr = at[p * N_STAGES + STAGE_FRONT], vm = at[p * N_STAGES + STAGE_VERIFY_MAIN],
                         ct = at[p * N_STAGES + STAGE_CTILDE];
            if (ea == NONE || fr == NONE || vm == NONE || ct == NONE) object("a stage that is never launched");
            if (!precedes(ea, vm)) object("expand_a(p) does not precede verify_main(p)");
            if (!precedes(fr, vm)) object("front(p) does not precede verify_main(p)");
            if (!precedes(vm, ct)) object("verify_main(p) does not precede ctilde(p)");
            if (p + 2 < n_parts[c] && !precedes(vm, at[(p + 2) * N_STAGES + STAGE_EXPAND_A])) object("verify_main(p) does not precede expand_a(p + 2)");
        }
    }
    // ---- call to call: one scratch
    for (size_t c = 0; c + 1 < n_parts.size(); c++)
        for (size_t i : stages_of[c])
            for (size_t j : stages_of[c + 1])
                if (!precedes(i, j)) object("a stage of a call does not precede a stage of the next call");
    return bad;
}

// ---------------------------------------------------------------------------------------------- the two shapes, written out
static bool same(const Step& a, Lane lane, Action act, Stage stage, size_t n) {
    return a.lane == lane && a.act == act && a.n == n && (act != ACT_LAUNCH || a.stage == stage);
}

static void check_one_part() {
    const OrderPlan o = order_plan(1);
    const StageLanes on = lanes_of_call(1);
    CHECK(on.expand_a == LANE_CALLER && on.arith == LANE_CALLER && on.front == LANE_VM);
    // caller: record fork | expand_a | wait front | verify_main | ctilde        vm: wait fork | front | record front
    // enqueued as: the fork, ExpandA, then the helper's wait and the front, so the front is dispatched behind ExpandA
    CHECK(o.n_events == 2 && o.steps.size() == 8);
    if (o.steps.size() != 8) return;
    const size_t fork = o.steps[0].n, front = o.steps[4].n;
    CHECK(fork != front && fork < o.n_events && front < o.n_events);
    CHECK(same(o.steps[0], LANE_CALLER, ACT_RECORD, N_STAGES, fork));
    CHECK(same(o.steps[1], LANE_CALLER, ACT_LAUNCH, STAGE_EXPAND_A, 0));
    CHECK(same(o.steps[2], LANE_VM, ACT_WAIT, N_STAGES, fork));
    CHECK(same(o.steps[3], LANE_VM, ACT_LAUNCH, STAGE_FRONT, 0));
    CHECK(same(o.steps[4], LANE_VM, ACT_RECORD, N_STAGES, front));
    CHECK(same(o.steps[5], LANE_CALLER, ACT_WAIT, N_STAGES, front));
    CHECK(same(o.steps[6], LANE_CALLER, ACT_LAUNCH, STAGE_VERIFY_MAIN, 0));
    CHECK(same(o.steps[7], LANE_CALLER, ACT_LAUNCH, STAGE_CTILDE, 0));
    // the same, property by property
    size_t caller_waits = 0, on_ea = 0;
    for (size_t i = 0; i < o.steps.size(); i++) {
        const Step& st = o.steps[i];
        on_ea += st.lane == LANE_EA;
        if (st.act == ACT_LAUNCH) CHECK(st.lane == (st.stage == STAGE_FRONT ? LANE_VM : LANE_CALLER));
        if (st.act == ACT_WAIT && st.lane == LANE_CALLER) {
            caller_waits++;
            // the event recorded right behind the front's launch
            bool found = false;
            for (size_t j = 1; j < i; j++)
                found |= o.steps[j].act == ACT_RECORD && o.steps[j].n == st.n && o.steps[j - 1].act == ACT_LAUNCH && o.steps[j - 1].stage == STAGE_FRONT &&
                         o.steps[j].lane == o.steps[j - 1].lane;
            CHECK(found);
        }
    }
    CHECK(caller_waits == 1 && on_ea == 0);
}

// Several parts: the schedule the three-stream pipeline was measured with (profiles/vfy_layer_ab.jsonl, kind `parts`), transcribed from
// its enqueue loop, less what ordered nothing: the arithmetic lane's own wait for the fork (its first step waits for ready[0], which is
// behind the fork) and the used[] records of the last two parts (no part p + 2 reads them).
static void check_several_parts(size_t n_parts) {
    const OrderPlan o = order_plan(n_parts);
    const StageLanes on = lanes_of_call(n_parts);
    CHECK(on.expand_a == LANE_EA && on.arith == LANE_VM && on.front == LANE_CALLER);
    struct Want { Lane lane; Action act; Stage stage; size_t n; };
    std::vector<Want> want;
    size_t n_events = 0;
    const size_t fork = n_events++;
    std::vector<size_t> used(n_parts, NONE);
    want.push_back({LANE_CALLER, ACT_RECORD, N_STAGES, fork});
    want.push_back({LANE_EA, ACT_WAIT, N_STAGES, fork});
    for (size_t i = 0; i < n_parts; i++) {
        if (i >= 2) want.push_back({LANE_EA, ACT_WAIT, N_STAGES, used[i - 2]});
        want.push_back({LANE_EA, ACT_LAUNCH, STAGE_EXPAND_A, i});
        const size_t ready = n_events++;
        want.push_back({LANE_EA, ACT_RECORD, N_STAGES, ready});
        want.push_back({LANE_CALLER, ACT_LAUNCH, STAGE_FRONT, i});
        const size_t front = n_events++;
        want.push_back({LANE_CALLER, ACT_RECORD, N_STAGES, front});
        want.push_back({LANE_VM, ACT_WAIT, N_STAGES, ready});
        want.push_back({LANE_VM, ACT_WAIT, N_STAGES, front});
        want.push_back({LANE_VM, ACT_LAUNCH, STAGE_VERIFY_MAIN, i});
        if (i + 2 < n_parts) {
            used[i] = n_events++;
            want.push_back({LANE_VM, ACT_RECORD, N_STAGES, used[i]});
        }
        want.push_back({LANE_VM, ACT_LAUNCH, STAGE_CTILDE, i});
    }
    const size_t join = n_events++;
    want.push_back({LANE_VM, ACT_RECORD, N_STAGES, join});
    want.push_back({LANE_CALLER, ACT_WAIT, N_STAGES, join});
    CHECK(o.n_events == n_events && o.steps.size() == want.size());
    // the same steps in the same order (events are numbered in the order of their records, here as there)
    for (size_t i = 0; i < want.size() && i < o.steps.size(); i++) CHECK(same(o.steps[i], want[i].lane, want[i].act, want[i].stage, want[i].n));
}

// ------------------------------------------------------------------------------------------------------------- the runs
static void check_calls(const std::vector<size_t>& n_parts) {
    std::vector<OrderPlan> calls;
    for (size_t np : n_parts) calls.push_back(order_plan(np));
    const int bad = objections(sequence(calls), n_parts, true);
    if (bad) std::fprintf(stderr, "  in calls of %zu%s parts\n", n_parts[0], n_parts.size() > 1 ? (" and " + std::to_string(n_parts[1])).c_str() : "");
    CHECK(bad == 0);
    // every record and every wait is needed: the checker objects to the calls without it
    for (size_t c = 0; c < calls.size(); c++)
        for (size_t i = 0; i < calls[c].steps.size(); i++) {
            const Step& st = calls[c].steps[i];
            if (st.act == ACT_LAUNCH) continue;
            if (objections(sequence(calls, c, i), n_parts, false) == 0) {
                std::fprintf(stderr, "call %zu of", c);
                for (size_t np : n_parts) std::fprintf(stderr, " %zu", np);
                std::fprintf(stderr, " parts: step %zu (%s %s, event %zu) orders nothing\n", i, st.act == ACT_RECORD ? "record" : "wait for", st.what, st.n);
                g_fail++;
            }
        }
    // and a launch left out is missed
    for (size_t c = 0; c < calls.size(); c++)
        for (size_t i = 0; i < calls[c].steps.size(); i++)
            if (calls[c].steps[i].act == ACT_LAUNCH) CHECK(objections(sequence(calls, c, i), n_parts, false) > 0);
}

int main() {
    const size_t sizes[4] = {1, 2, 3, 7};
    CHECK(order_plan(0).steps.empty() && order_plan(0).n_events == 0);
    check_one_part();
    for (size_t np : sizes)
        if (np > 1) check_several_parts(np);
    for (size_t a : sizes) {
        check_calls({a});
        for (size_t b : sizes) check_calls({a, b});
    }
    // the checker itself: the front enqueued on the caller's lane of a one-part chain needs no event at all, and a front that nothing
    // folds back is objected to
    {
        const OrderPlan chain = order_plan(1, StageLanes{LANE_CALLER, LANE_CALLER, LANE_CALLER});
        CHECK(chain.n_events == 1 && chain.steps.size() == 5);  // (the fork record alone: nobody waits for it, which the checker says)
        CHECK(objections(sequence({chain}), {1}, false) == 1);
        OrderPlan loose = order_plan(1);
        loose.steps.erase(loose.steps.begin() + 4, loose.steps.begin() + 6);  // record front, wait front
        CHECK(objections(sequence({loose}), {1}, false) >= 2);  // front(0) precedes neither verify_main(0) nor the caller's end
    }
    if (g_fail) {
        std::fprintf(stderr, "vfy_order: %d checks failed\n", g_fail);
        return 1;
    }
    std::puts("vfy_order OK");
    return 0;
}

// The part plan, the scratch carve and the order plan of mldsa_vfy_verify as pure host code (no HIP here: tests/cpp/vfy_parts_main.cpp
// and tests/cpp/vfy_order_main.cpp compile it alone, under the sanitizers).  A call of n_ops ops is cut into parts of `part` ops (the last
// one may be shorter); part i writes its A_hat into half i & 1 of a two-part ring, everything else is one row per op of the call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mldsa_vfy {

constexpr size_t PACKED_POLY_BYTES = 768;  // the core's 24-bit A_hat row (field.h PACKED_POLY_DWORDS)
constexpr size_t CARVE_ALIGN = 256;

struct Part {
    size_t first = 0, count = 0;  // ops [first, first + count) of the call
    int half = 0;                 // the ring half its A_hat lives in
};

// PartPlan plan(n_ops, part); for (i < plan.n_parts()) plan.at(i)  -- every op in exactly one part, in order; none for an empty call
struct PartPlan {
    size_t n_ops, part;
    PartPlan(size_t n_ops_, size_t part_) : n_ops(n_ops_), part(part_ ? part_ : 1) {}
    size_t n_parts() const { return n_ops / part + (n_ops % part ? 1 : 0); }
    // ring halves in use: a call of one part needs one
    size_t halves() const { return n_parts() > 1 ? 2 : n_parts(); }
    // ops a ring half holds
    size_t half_ops() const { return n_ops < part ? n_ops : part; }
    Part at(size_t i) const {
        Part p;
        p.first = i * part;
        p.count = n_ops - p.first < part ? n_ops - p.first : part;
        p.half = (int)(i & 1);
        return p;
    }
};

// byte offsets into a CARVE_ALIGN-aligned scratch; every array starts CARVE_ALIGN-aligned
struct Carve {
    size_t ring[2];  // A_hat of a part: half_ops * k * l packed rows (ring[1] == ring[0] when the call is one part)
    size_t ring_bytes;
    size_t c;        // c as one byte per coefficient: 256 bytes per op
    size_t znorm, hvalid, ctx_bad, key_bad, kidx;  // one dword per op
    size_t mu_w1;    // rows of mu | w1: 64 + w1_len bytes per op
    size_t bytes;    // the whole scratch
};

inline size_t carve_up(size_t x) { return (x + CARVE_ALIGN - 1) / CARVE_ALIGN * CARVE_ALIGN; }

inline Carve carve(int k, int l, size_t w1_len, const PartPlan& plan) {
    Carve c;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += carve_up(bytes);
        return here;
    };
    c.ring_bytes = plan.half_ops() * (size_t)(k * l) * PACKED_POLY_BYTES;
    c.ring[0] = take(c.ring_bytes);
    c.ring[1] = plan.halves() > 1 ? take(c.ring_bytes) : c.ring[0];
    c.c = take(plan.n_ops * 256);
    c.znorm = take(plan.n_ops * 4);
    c.hvalid = take(plan.n_ops * 4);
    c.ctx_bad = take(plan.n_ops * 4);
    c.key_bad = take(plan.n_ops * 4);
    c.kidx = take(plan.n_ops * 4);
    c.mu_w1 = take(plan.n_ops * (64 + w1_len));
    c.bytes = at + CARVE_ALIGN;  // (the slack of the core's own carve, pipeline.hip VerifyWs)
    return c;
}

// ------------------------------------------------------------------------------------------------------------ the order of a call
// What mldsa_vfy_verify enqueues, as data: enqueue() (vfy.hip) walks the list and issues one call of the runtime per step, and
// tests/cpp/vfy_order_main.cpp derives from the same list what is ordered behind what.  A lane is a FIFO: the caller's stream or one of
// the library's two.  An event orders a lane behind the point of another lane where it was recorded.
enum Lane { LANE_CALLER = 0, LANE_EA = 1, LANE_VM = 2, N_LANES = 3 };
enum Action { ACT_RECORD, ACT_WAIT, ACT_LAUNCH };
// front: k_sanitize_keys, k_mu, k_sample_in_ball; ctilde: the c~ hash and the verdict
enum Stage { STAGE_EXPAND_A = 0, STAGE_FRONT = 1, STAGE_VERIFY_MAIN = 2, STAGE_CTILDE = 3, N_STAGES = 4 };

struct Step {
    Lane lane;
    Action act;
    Stage stage;       // ACT_LAUNCH: what is launched (for the other actions: the stage the event belongs to)
    size_t n;          // ACT_LAUNCH: the part; ACT_RECORD, ACT_WAIT: the event, below OrderPlan::n_events
    const char* what;  // for the message of a failed step
};

struct OrderPlan {
    std::vector<Step> steps;  // in the order they are enqueued
    size_t n_events = 0;
};

// Where the stages of a call of n_parts parts run.  One part has nothing to overlap: ExpandA, k_verify_main and the c~ hash are one chain
// on the caller's stream and the front runs on a library stream beside it.  Several parts: ExpandA of part p + 1 on one library stream
// beside k_verify_main and the c~ hash of part p on the other, the fronts on the caller's stream.
struct StageLanes {
    Lane expand_a, arith, front;
};
inline StageLanes lanes_of_call(size_t n_parts) {
    return n_parts == 1 ? StageLanes{LANE_CALLER, LANE_CALLER, LANE_VM} : StageLanes{LANE_EA, LANE_VM, LANE_CALLER};
}

// The steps of a call of n_parts parts with its stages on the lanes `on`.  Per part, in enqueue order: ExpandA, the front, k_verify_main,
// the c~ hash.  An event is spent only where the two ends of an order are on different lanes, and only where no other path gives it:
//   fork          the caller's stream at the call -> the first launch of every other lane that launches ahead of any wait
//   ready[p]      ExpandA(p) -> k_verify_main(p)
//   front[p]      front(p) -> k_verify_main(p)
//   used[p]       k_verify_main(p) -> ExpandA(p + 2), which writes the ring half it read
//   join          the arithmetic lane's end -> the caller's stream
// A lane other than the arithmetic one is folded back through ready[] / front[]; the arithmetic lane through the join, unless it IS the
// caller's stream.  One part on lanes_of_call(1):
//   caller: record fork | expand_a | wait front | verify_main | ctilde
//   vm:     wait fork | front | record front
// ExpandA is enqueued ahead of the front, so the front is dispatched behind it.
inline OrderPlan order_plan(size_t n_parts, const StageLanes& on) {
    OrderPlan o;
    if (n_parts == 0) return o;
    const size_t none = (size_t)-1;
    auto put = [&o](Lane lane, Action act, Stage stage, size_t n, const char* what) { o.steps.push_back(Step{lane, act, stage, n, what}); };
    const size_t fork = o.n_events++;
    bool forked[N_LANES] = {true, false, false};  // the lane is behind the fork
    auto reach = [&](Lane lane, Stage stage) {
        if (!forked[lane]) put(lane, ACT_WAIT, stage, fork, "the fork");
        forked[lane] = true;
    };
    // record in `from` and wait in `to`, in two halves: the wait is enqueued where the consumer is
    auto record = [&](Lane from, Lane to, Stage stage, const char* what) {
        if (from == to) return none;
        put(from, ACT_RECORD, stage, o.n_events, what);
        return o.n_events++;
    };
    auto wait = [&](Lane to, size_t event, Stage stage, const char* what) {
        if (event == none) return;
        put(to, ACT_WAIT, stage, event, what);
        forked[to] = true;  // (behind a lane that was)
    };
    put(LANE_CALLER, ACT_RECORD, STAGE_EXPAND_A, fork, "the fork");
    std::vector<size_t> used(n_parts, none);
    for (size_t p = 0; p < n_parts; p++) {
        if (p >= 2) wait(on.expand_a, used[p - 2], STAGE_EXPAND_A, "the ring half");
        reach(on.expand_a, STAGE_EXPAND_A);
        put(on.expand_a, ACT_LAUNCH, STAGE_EXPAND_A, p, "k_expand_a launch");
        const size_t ready = record(on.expand_a, on.arith, STAGE_EXPAND_A, "ExpandA's end");
        reach(on.front, STAGE_FRONT);
        put(on.front, ACT_LAUNCH, STAGE_FRONT, p, "front launch");
        const size_t front = record(on.front, on.arith, STAGE_FRONT, "the front's end");
        wait(on.arith, ready, STAGE_EXPAND_A, "ExpandA");
        wait(on.arith, front, STAGE_FRONT, "the front");
        reach(on.arith, STAGE_VERIFY_MAIN);
        put(on.arith, ACT_LAUNCH, STAGE_VERIFY_MAIN, p, "k_verify_main launch");
        if (p + 2 < n_parts) used[p] = record(on.arith, on.expand_a, STAGE_VERIFY_MAIN, "the end of the ring half's use");
        put(on.arith, ACT_LAUNCH, STAGE_CTILDE, p, "k_ctilde_verdict launch");
    }
    // the last ExpandA and the last front precede the last k_verify_main: the arithmetic lane's end is the call's end
    wait(LANE_CALLER, record(on.arith, LANE_CALLER, STAGE_CTILDE, "the join"), STAGE_CTILDE, "the join");
    return o;
}

inline OrderPlan order_plan(size_t n_parts) { return order_plan(n_parts, lanes_of_call(n_parts)); }

}  // namespace mldsa_vfy

// refine_cadence.h - the refinement cadence of the single solve (pure host code: no device, no handle, no allocation)
//
// Every single solve decides how many correction passes its graph carries, whether it takes a residual at all, and
// whether its verdict is left to the next tree launch.  The state behind those decisions is here, grouped by lifetime,
// and every change of it is one of the transitions of `Cadence` below; the runtime (runtime_queue.inc) calls them where
// the events happen and hipfact_debug_refine_cadence replays a script of events through them (tests: no GPU needed).
// The option values go in as CadenceKnobs, what the host sees of the pinned control block as a CtlPeek: nothing here
// reads an option, pinned memory or the device.
#pragma once

#include <algorithm>

namespace hipfact {

struct CadenceKnobs {
  int refine_steps;  // correction passes inside the solve graph (0: no residual at all)
  bool refine_adaptive;
  int check_every, check_backoff, check_max;  // refine_check_*
  bool decide_lazy, factor_hint_peek;
};

// the host's copy of the control block: seq counts the first residuals the device has judged
struct CtlPeek {
  int seq, done, status, iters;
  double omega, tol;
};
// The judgement "well conditioned": the first pass alone met a quarter of the tolerance.
inline bool first_pass_sufficed(const CtlPeek& c) { return c.done && c.status == 0 && c.iters == 0 && c.omega <= 0.25 * c.tol; }

// Per factorisation of a plan (parks with the plan).
struct FactorCadence {
  int refine_inline = 1;     // correction passes currently carried by the solve graphs
  bool inline_probe = true;  // the first solve of this factorisation has not been looked at yet
  bool wc_hint = false;      // the previous factorisation of this plan was judged well-conditioned (first pass enough)
};
// Per plan: where its factorisations stand in the handle's solve_seq.  Never put back.
struct PlanCadence {
  int seq_at_factor = 0;      // solve_seq at the time of the last factorisation
  int hint_seq_seen = -1;     // the last verdict a refactorisation has looked at (factor_hint_peek)
  int first_factor_seq = -1;  // solve_seq at the first factorisation of this plan (verdicts behind it belong to its factorisations)
};
// Per handle, remembered between solves.  Once a factorisation has been judged well-conditioned (no correction pass in
// its solve graphs), the residual of K z = b is checked on every k-th solve only.
struct SolveCadence {
  int check_interval_now = 0;      // the interval in force (< 1: reload refine_check_every; back to it with every factorisation)
  long solves_since_check = 0;
  bool last_solve_checked = true;  // the last solve carried a residual (and possibly correction passes)
  long num_checked = 0, num_refined = 0, num_passes = 0;  // residuals taken / solves that applied a pass / passes applied
};
// Per handle, advanced by every solve, remembered or not.
struct LiveCadence {
  bool ctl_pending = false;      // the control block of the last checked solve has not been looked at yet
  bool decide_deferred = false;  // a verdict left to the next tree launch is outstanding
  int solve_seq = 0;             // solves with a residual queued since the control block was last cleared
};

// What a solve about to be queued has decided (Cadence::solve_decision).
struct SolveDecision {
  bool defer;        // its verdict is left to the next tree launch
  bool unchecked;    // no residual
  bool flush_first;  // a pending verdict has no tree launch to deliver it: launch it, then Cadence::verdict_flushed
  int passes;        // correction passes in its graph (a checked solve)
  int key;           // of its captured sequence, without the top-block term: passes, -2 deferred, -1 without a residual
};

// What solves that are not to be remembered (the columns of multi_single_cols, the plain solves of the extra-precise
// solve) save in front of them and put back behind them: Cadence::save / put_back.
struct SavedCadence {
  FactorCadence f;
  SolveCadence s;
};

// The four parts where they live (the handle: two with the active plan state, two on the handle itself).
struct Cadence {
  FactorCadence& f;
  PlanCadence& p;
  SolveCadence& s;
  LiveCadence& l;

  bool verdict_unread() const { return l.ctl_pending; }
  bool verdict_outstanding() const { return l.decide_deferred; }
  int passes_in_graph() const { return f.refine_inline; }
  bool last_checked() const { return s.last_solve_checked; }
  // judge(well): no correction pass in the solve graphs of this factorisation - or (well = false: the judgement
  // withdrawn) a pass again.  Called by the transitions below and by the device loops when their last projection fails.
  void judge(const CadenceKnobs& k, bool well) {
    f.wc_hint = well;
    f.refine_inline = well ? 0 : std::max(f.refine_inline, std::min(k.refine_steps, 1));
  }

  // Factorisation queued (factor_async, behind a launch that succeeded; graphed: the captured sequence, which has
  // delivered a pending verdict itself).  A plan whose previous factorisation needed no correction pass starts without
  // one; a caller that solves ONCE per factorisation and never synchronises never reaches the peek of the second solve:
  // the last verdict that has come back for a factorisation of this plan (`peek`, nobody has looked at it yet) stands in.
  void factor_queued(const CadenceKnobs& k, bool graphed, const CtlPeek& peek) {
    if (graphed) l.decide_deferred = false;
    l.ctl_pending = false;
    if (p.first_factor_seq < 0) p.first_factor_seq = l.solve_seq;
    if (k.factor_hint_peek && k.refine_adaptive && k.refine_steps > 0 && peek.seq > p.first_factor_seq && peek.seq > p.hint_seq_seen) {
      p.hint_seq_seen = peek.seq;
      f.wc_hint = first_pass_sufficed(peek);
    }
    f.refine_inline = (f.wc_hint && k.refine_adaptive) ? 0 : k.refine_steps;
    f.inline_probe = true;
    p.seq_at_factor = l.solve_seq;
    s.solves_since_check = 0;
    s.check_interval_now = k.check_every;
  }

  // Solve about to be queued (solve_async).  wants_peek: has the previous solve of this factorisation still to be
  // judged?  Only then does the caller read the pinned copy.
  bool wants_peek(const CadenceKnobs& k) const {
    return k.refine_steps > 0 && k.refine_adaptive && f.inline_probe && l.solve_seq > p.seq_at_factor;
  }
  // tree_delivers: the tree launch of this solve delivers pending verdicts; peek: the pinned copy (wants_peek) or
  // anything with another seq; all_checked: every solve of the caller's call takes a residual, whatever the interval.
  // If the first pass of the previous solve met the tolerance with room to spare, this and the following solves drop the
  // correction pass and defer their verdict; of those, every check_interval_now-th takes a residual, and the interval
  // grows while the checks keep passing (what a check guards against shows on the first solves of a factorisation).
  SolveDecision solve_decision(const CadenceKnobs& k, bool tree_delivers, const CtlPeek& peek, bool all_checked = false) {
    if (wants_peek(k) && peek.seq == l.solve_seq) {
      judge(k, first_pass_sufficed(peek));
      f.inline_probe = false;
    }
    SolveDecision d;
    d.defer = k.decide_lazy && k.refine_steps > 0 && k.refine_adaptive && f.refine_inline == 0 && tree_delivers;
    if (s.check_interval_now < 1) s.check_interval_now = k.check_every;
    d.unchecked = !all_checked && d.defer && (!f.inline_probe || f.wc_hint) && s.check_interval_now > 1 &&
                  (s.solves_since_check % s.check_interval_now) != 0;
    if (!all_checked && !d.unchecked && k.check_every > 1 && s.solves_since_check >= s.check_interval_now && k.check_backoff > 1)
      s.check_interval_now = std::min(std::max(k.check_max, k.check_every), s.check_interval_now * k.check_backoff);
    s.solves_since_check = d.unchecked ? s.solves_since_check + 1 : 1;
    s.num_checked += (!d.unchecked && k.refine_steps > 0);
    s.last_solve_checked = !d.unchecked;
    d.flush_first = !tree_delivers && l.decide_deferred;
    d.passes = f.refine_inline;
    d.key = k.refine_steps > 0 ? (d.defer ? -2 : f.refine_inline) : -1;
    return d;
  }
  // A pending verdict has been launched on its own (flush_decide).
  void verdict_flushed() { l.decide_deferred = false; }
  // Solve queued (behind its launch, when that succeeded).
  void solve_queued(const CadenceKnobs& k, const SolveDecision& d) {
    if (!d.unchecked) l.decide_deferred = d.defer;  // (the tree launch of this solve has delivered an older one)
    if (k.refine_steps > 0 && !d.unchecked) l.solve_seq++;
    l.ctl_pending = k.refine_steps > 0 && (!d.unchecked || l.ctl_pending);
  }

  // Verdict read (finish_solve, behind its continuation loop, c: the final control block): the first solve of a
  // factorisation is judged here instead of at the next solve's peek.
  void verdict_read(const CadenceKnobs& k, const CtlPeek& c) {
    l.ctl_pending = false;
    if (f.inline_probe && k.refine_adaptive && k.refine_steps > 0) {
      if (first_pass_sufficed(c)) judge(k, true);
      f.inline_probe = false;
    }
  }
  // ... and counted, once finish_solve knows that the solve stands (no retry on another plan); continued: the rounds
  // of passes the host added.  The next solves of this factorisation carry as many passes as this one needed.
  void verdict_counted(const CtlPeek& c, int continued) {
    if (c.iters > 0) s.num_refined++;
    s.num_passes += c.iters;
    if (continued > 0) {
      f.refine_inline = std::min(std::max(f.refine_inline, c.iters), 4);
      f.wc_hint = false;
    }
  }

  // The device loops run their projections without a residual check: only on a factorisation that has been judged.
  bool unchecked_solves_ok(const CadenceKnobs& k) const {
    return k.refine_steps == 0 || (k.refine_adaptive && f.refine_inline == 0 && !f.inline_probe);
  }
  // The device counted a first residual that no solve queued (the verified last projection of a device loop).
  void counted_device_residual() { l.solve_seq++; }

  // Slots reset (reset_dataflow_state: the control block is zero again).
  void slots_reset() {
    l.solve_seq = p.seq_at_factor = 0;
    l.ctl_pending = false;
  }

  // The option setters: refine_steps reloads the passes of the active factorisation, refine_check_every and
  // refine_check_backoff make the next solve reload the interval.
  void steps_set(const CadenceKnobs& k) { f.refine_inline = k.refine_steps; }
  void check_interval_set() { s.check_interval_now = 0; }

  // In front of solves that are not to be remembered, and behind them.  Everything saved goes back, with ONE exception:
  // a factorisation not yet judged when saved (inline_probe) keeps the judgement found since, and inline_probe itself
  // is never put back.  The plan's seq markers and the live part are not saved: such solves really advance them.
  SavedCadence save() const { return SavedCadence{f, s}; }
  void put_back(const SavedCadence& saved) {
    s = saved.s;
    if (!saved.f.inline_probe) {
      f.refine_inline = saved.f.refine_inline;
      f.wc_hint = saved.f.wc_hint;
    }
  }
};

}  // namespace hipfact

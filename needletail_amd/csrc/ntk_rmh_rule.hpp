// The guess / accept / raise rule of the per-record MinHash sketches (ntk_record_minhash.hip; include/needletail_amd_record_minhash.h),
// for bottom-s sketches: a record's threshold is guessed from its length, verified after the round, and raised where it was too low.
// Plain C++ without any device call, so that it also compiles with g++: the CPU suite walks it exhaustively (tests/test_rmh_rule.py).
// The functions are constexpr, which is what lets the device code call them as they stand.
//
// A round appends, for every window of record r, the hash h with lo[r] <= h <= tau[r] (lo is 0 in the first round).  Afterwards the
// record holds EVERY occurrence of every hash <= tau[r].  Accepted iff tau[r] == ~0 (it holds everything) or it holds at least num
// distinct hashes: the num smallest of the record are then among them, with all their occurrences.  Otherwise what it holds stays,
// lo[r] becomes tau[r] + 1 and tau[r] is raised: the next round adds exactly the hashes in between, so no occurrence is taken twice.
#pragma once

#include <stdint.h>

constexpr uint64_t kRmhAll = ~(uint64_t)0;
constexpr uint64_t kRmhAllPass = 4;      // NTK_RECORD_MINHASH_ALLPASS
constexpr uint64_t kRmhMinRaise = 4;     // a raise multiplies the threshold by at least this: at most 32 raises reach ~0

// hashes expected at or below a guessed threshold: twice what is needed, and 16 more so that small num are safe too (the number that
// passes is close to Poisson: its mean 2 num + 16 lies more than 4 standard deviations above num for every num >= 1, 22 for num = 1000)
constexpr uint64_t rmh_want(uint64_t num) { return 2 * num + 16; }

// The first threshold of a record of n_ends candidate window ends: ~0 (everything passes) where the record is short, else the hash
// below which rmh_want(num) of n_ends uniformly spread hashes are expected.  Monotone: a longer record never gets a higher threshold.
constexpr uint64_t rmh_guess(uint64_t n_ends, uint64_t num)
{
    if (n_ends <= kRmhAllPass * num || n_ends <= rmh_want(num)) return kRmhAll;
    return (kRmhAll / n_ends) * rmh_want(num);   // want < n_ends: no overflow
}

// a record that holds `distinct` hashes, all those <= tau: are its num smallest exact?
constexpr bool rmh_accept(uint64_t tau, uint64_t distinct, uint64_t num) { return tau == kRmhAll || distinct >= num; }

// The next threshold of a record that was not accepted (tau != ~0, distinct < num): the old one times the shortfall the round showed -
// rmh_want(num) were hoped for and `distinct` came - and at least times kRmhMinRaise; ~0 where that overflows or nothing came at all.
// Strictly above tau.
constexpr uint64_t rmh_raise(uint64_t tau, uint64_t distinct, uint64_t num)
{
    if (distinct == 0) return kRmhAll;
    uint64_t factor = (rmh_want(num) + distinct - 1) / distinct;
    if (factor < kRmhMinRaise) factor = kRmhMinRaise;
    const uint64_t base = tau ? tau : 1;
    return base > kRmhAll / factor ? kRmhAll : base * factor;
}

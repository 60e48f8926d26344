"""The mutant list of the tile logic: small wrong edits to the headers that the CPU suite compiles with g++ (csrc/ntk_tile.hpp through
tests/emu/, and the host arithmetic of ntk_plan.hpp, ntk_chunks.hpp, ntk_compat_plan.hpp, ntk_trim_runs.hpp).  tools/mutation_audit.py
applies them one at a time to a copy of the tree and runs the CPU tests on it: a mutant that passes shows that no input of the shared
generators (tests/_seams.py, tests/_mutant_inputs.py) tells the right logic from the wrong one there, and the device sweeps built on those
inputs cannot either.  tests/test_tile_mutants.py keeps the list in step with the sources.  Data only: nothing here is compiled or run on a
device, and no edit lies inside a __HIP_DEVICE_COMPILE__ branch (the emulator would not see it; tests/test_gpu_tile_helpers.py ties those).

A mutant: id; file (under needletail_amd/csrc/); anchor (occurs exactly once in the file); replacement; function; group; the CPU test
files that cover the function (run first); a one-line note; equivalent (no input can tell the two apart - the note holds the argument).
Edits are single-token: a relational boundary, a shift or constant off by one or two, a tie rule swapped, a mask polarity, a dropped term,
swapped strand operands, tail handling."""
from collections import namedtuple

Mutant = namedtuple("Mutant", "id file anchor replacement function group tests note equivalent")

TILE, PLAN, CHUNKS, COMPAT, TRIM = "ntk_tile.hpp", "ntk_plan.hpp", "ntk_chunks.hpp", "ntk_compat_plan.hpp", "ntk_trim_runs.hpp"
TL, MS, WS, XS, QW = ("tests/test_tile_logic_emu.py", "tests/test_minimizer_seams_emu.py", "tests/test_wide_seams_emu.py",
                      "tests/test_exact_stride_emu.py", "tests/test_quality_watch.py")
MI = "tests/test_mutant_inputs_emu.py"   # the inputs added for the survivors of the first audit (tests/_mutant_inputs.py)
CH, CP, TR = "tests/test_chunks.py", "tests/test_compat_plan.py", "tests/test_trim_abi.py"

# the emulator test files: after a mutant's covering files the audit runs the rest of these
EMU_TEST_FILES = (TL, MI, MS, WS, XS, QW)
# headers an emulator source includes: only their mutants can fail an emulator test that is not in the covering list
EMU_HEADERS = (TILE, PLAN)

GROUPS = {   # group -> the least number of mutants
    "encode": 10, "masks": 12, "strand": 10, "minimizer": 15, "wide": 8, "host": 8,
}

_M = []


def _m(id, file, function, group, tests, anchor, replacement, note, equivalent=False):
    _M.append(Mutant(id, file, anchor, replacement, function, group, tuple(tests), note, equivalent))


# ---- the eight of the trial --------------------------------------------------------------------------------------------------------------
_m("wk_strand_tie_false", TILE, "wk_strand", "wide", (TL, WS),
   "lt = F2 < V2; tie = F2 == V2;", "lt = F2 < V2; tie = false;",
   "a window equal to its reverse complement over 32 bases no longer raises the redo flag")
_m("keyg_min_le", TILE, "key_min(KeyG)", "minimizer", (TL, MS),
   "const bool t = r.v < l.v;", "const bool t = r.v <= l.v;",
   "ties go to the rightmost k-mer")
_m("keys_f64_j8", TILE, "minimizer_keys_f64", "minimizer", (TL, MS),
   "if (j <= 9) {", "if (j <= 8) {",
   "position 9 takes the shifted-window form, whose low word lacks the bits of the lane before")
_m("wk_valid16_thr_minus1", TILE, "wk_valid16", "wide", (TL, WS),
   "const int32_t thr = before + (int32_t)k - 16 * slot;", "const int32_t thr = before + (int32_t)k - 1 - 16 * slot;",
   "the window that still holds the break is emitted")
_m("wk_stage_last_break_highest", TILE, "wk_stage_slot", "wide", (TL, WS),
   "16 * slot + 15 - (int32_t)__builtin_ctz(r.bad)", "16 * slot + (int32_t)__builtin_clz(r.bad) - 16",
   "the slot reports its first break as its last")
_m("or_bytes_nb_gt4", TILE, "or_of_input_bytes", "encode", (QW, MI),
   "r |= nb >= 4 ? w[d]", "r |= nb > 4 ? w[d]",
   "a dword that holds exactly its four input bytes is masked to none (1u << 32)")
_m("or_bytes_keep15", TILE, "or_of_input_bytes", "encode", (QW, MI),
   "if (keep >= 16) return raw.x | raw.y | raw.z | raw.w;", "if (keep >= 15) return raw.x | raw.y | raw.z | raw.w;",
   "the padding byte behind a line of 15 input bytes is watched")
_m("min_invalid_halo_not_forced", TILE, "minimizer_invalid16", "minimizer", (TL, MS),
   "inval = lane < (uint32_t)kHaloLanes ? 0xFFFFu : ((uint32_t)bw & 0xFFFFu);", "inval = ((uint32_t)bw & 0xFFFFu);",
   "EQUIVALENT.  The k-mer-invalid bits of lanes 0 and 1 (tile positions p <= 31) are smeared over the window ends p .. p + w - 1 <= "
   "30 + w (the shifts of min_smear add up to w - 1).  The first emitting lane is min_halo_lanes = 2 + ceil((w - 1) / 16), its first "
   "window end 32 + 16 ceil((w - 1) / 16) >= 31 + w: no bit of lanes 0 / 1 reaches an emitted window, and the ends below it are set to "
   "0xFFFF by the `lane < a.min_halo_lanes` mask of the return whatever they held.  The line is redundant (a candidate for deletion in a "
   "later change); the one-smear branch has never had it.", equivalent=True)

# ---- encode, quality, lower-case watch ---------------------------------------------------------------------------------------------------
_m("quality_cut_sel_lt128", TILE, "quality_cut", "encode", (QW, TL),
   "c.sel = cutoff <= 128 ? 0xFFFFFFFFu : 0u;", "c.sel = cutoff < 128 ? 0xFFFFFFFFu : 0u;",
   "cutoff 128 takes the AND form: every quality compares as below it")
_m("quality_cut_255", TILE, "quality_cut", "encode", (QW, TL),
   "128u - cutoff : 256u - cutoff)", "128u - cutoff : 255u - cutoff)",
   "cutoffs above 128 compare one too high")
_m("quality_break_polarity", TILE, "quality_break", "encode", (QW, TL),
   "return bitop3<0xF2>(s, ge, 0x80808080u);", "return bitop3<0xF8>(s, ge, 0x80808080u);",
   "s | (ge & 0x80..): the good bases are masked, the bad ones kept")
_m("lower_watch_shift1", TILE, "lower_watch_or", "encode", (QW,),
   "return bitop3<0xF4>(lc, m, m >> 2); }", "return bitop3<0xF4>(lc, m, m >> 1); }",
   "bit 6 instead of bit 7 clears the watch: no letter is watched")
_m("encode16_rcode_swapped", TILE, "encode16", "encode", (TL,),
   "r.rcode = bfi(0x55555555u, t >> 1, t << 1);", "r.rcode = bfi(0x55555555u, t << 1, t >> 1);",
   "the bit pairs of the reverse-complement word stay reversed")
_m("encode16_bad_mask_7fff", TILE, "encode16", "encode", (TL,),
   "r.bad = or_and(g, g >> 8, 0xFFFFu);", "r.bad = or_and(g, g >> 8, 0x7FFFu);",
   "a break at byte 0 of a line is not seen")
_m("encode_sv2_u_on_bit_path", TILE, "encode16_sv2", "encode", (TL, XS),
   "kLutHi = ACCEPT_U ? 0x47FF5554u : 0x47FFFF54u;", "kLutHi = ACCEPT_U ? 0x47FF5554u : 0x47FF5554u;",
   "U is a base where the input is not read as normalised")
_m("encode_sv2_fold_byte0", TILE, "encode16_sv2", "encode", (TL, XS),
   "r.uu[i] = w[i] & 0xDFDFDFDFu;", "r.uu[i] = w[i] & 0xDFDFDFFFu;",
   "a lower-case base in byte 0 of a dword is a break")
_m("bad16_weights_d2", TILE, "bad16_from_letters", "encode", (TL, MS),
   "const uint32_t wt = (d & 1) ? 0x01020408u : 0x10204080u;", "const uint32_t wt = (d & 2) ? 0x01020408u : 0x10204080u;",
   "the flags of dwords 1 and 2 swap their weights")
_m("bad16_hi_d1", TILE, "bad16_from_letters", "encode", (TL, MS),
   "if (d < 2) hi = dot4(nz, wt, hi);", "if (d < 1) hi = dot4(nz, wt, hi);",
   "dword 1 adds its flags to the low half")

# ---- window masks and geometry -----------------------------------------------------------------------------------------------------------
_m("set_k_mask_hi_31", TILE, "scan_args_set_k", "masks", (TL,),
   "((1u << (2 * k - 32)) - 1u);", "((1u << (2 * k - 31)) - 1u);",
   "the high word keeps one bit of the base before the k-mer")
_m("set_k_bin_p5", TILE, "scan_args_set_k", "masks", (TL,),
   "const uint32_t p = k < 6 ? k : 6;", "const uint32_t p = k < 5 ? k : 6;",
   "k = 5 bins by six bases it does not have")
_m("set_k_smear_four_rounds", TILE, "scan_args_set_k", "masks", (TL,),
   "    for (int i = 0; i < 5; i++) {\n        uint32_t s = len < k", "    for (int i = 0; i < 4; i++) {\n        uint32_t s = len < k",
   "the fifth smear round (k - 16 for k > 16) is dropped: a break invalidates only the 16 windows that follow it")
_m("stride_three_halo_from_34", TILE, "sv2_stride_bytes", "masks", (TL, MS),
   "return km > 32 ? 61 * 16", "return km > 33 ? 61 * 16",
   "a window of 33 bytes advances by 62 lanes while three are halo")
_m("geom_keep_lane0", TILE, "Sv2Geom", "masks", (XS, TL),
   "kKeep = ~((1ull << kHalo) - 1ull);", "kKeep = ~((1ull << kHalo) - 2ull);",
   "lane 0 emits the windows that lie inside it: emitted twice")
_m("masks_ab_c16", TILE, "window_masks_ab", "masks", (TL, XS),
   "const int c = 17 + j - K, a_ = c > 0 ? c : 0;", "const int c = 16 + j - K, a_ = c > 0 ? c : 0;",
   "the previous lane's suffix starts one byte early")
_m("masks_ab_overlap_le", TILE, "window_masks_ab", "masks", (XS,),
   "if (c >= 0 && c < kOverlap) v &= ~2ull;", "if (c >= 0 && c <= kOverlap) v &= ~2ull;",
   "one window more of lane 1 is left to a previous tile that does not emit it")
_m("masks_ab_halo_lane1_kept", TILE, "window_masks_ab", "masks", (TL,),
   "A[0] = EXACT ? G[0] : G[0] & ~3ull;", "A[0] = EXACT ? G[0] : G[0] & ~1ull;",
   "halo lane 1 emits")
_m("masks1_first_byte_plus2", TILE, "window_masks1_ab", "masks", (TL, XS),
   "const int a = j - K + 1;   // first byte of the window", "const int a = j - K + 2;   // first byte of the window",
   "windows of 9 .. 16 bytes are tested one byte short")
_m("masks1_suffix_halo_all", TILE, "window_masks1_ab", "masks", (TL, XS),
   "else if (j == 15) { A[j] = S[a & 15]; B[j] = kNoHalo; }", "else if (j == 15) { A[j] = S[a & 15]; B[j] = kAll; }",
   "the halo lanes emit the window ending at their byte 15")
_m("masks1_short_own_byte0", TILE, "window_masks1_ab", "masks", (TL, XS),
   "E[16] &= kNoHalo;  // cleared in own byte 0", "E[16] &= kAll;  // cleared in own byte 0",
   "the halo lanes emit the windows over their byte 0 (k <= 8)")
_m("masks1_short_j_gt_k", TILE, "window_masks1_ab", "masks", (TL, XS),
   "B[j] = j >= K ? kNoHalo : kAll;", "B[j] = j > K ? kNoHalo : kAll;",
   "k a power of two: the halo lanes emit the window ending at byte k")
_m("masks_span_j_lt_c", TILE, "window_masks_span", "masks", (TL,),
   "if (j <= C) B[j] = (S[(15 - C + j) & 15] << (q + 1)) & Fq;", "if (j < C) B[j] = (S[(15 - C + j) & 15] << (q + 1)) & Fq;",
   "the window ending at byte C misses the last byte of the lane q + 1 back")
_m("masks_runtime_q", TILE, "window_masks_runtime", "masks", (TL,),
   "const uint32_t q = (L - 2) >> 4;", "const uint32_t q = (L - 1) >> 4;",
   "L = 17 + 16 n asks for one whole lane too many")

# ---- strand choice and emit --------------------------------------------------------------------------------------------------------------
_m("lane_tile_tie_two_words", TILE, "lane_tile", "strand", (MI, TL),
   "take_fwd = TIE_RC ? (f < r) : (f <= r);", "take_fwd = TIE_RC ? (f <= r) : (f <= r);",
   "byte path, k >= 17: a k-mer equal to its reverse complement reports forward")
_m("lane_tile_tie_one_word", TILE, "lane_tile", "strand", (MI, TL),
   "take_fwd = TIE_RC ? (fl < rl) : (fl <= rl);", "take_fwd = TIE_RC ? (fl < rl) : (fl < rl);",
   "bit path, k <= 16: a k-mer equal to its reverse complement reports the reverse complement")
_m("lane_tile_halo_7fff", TILE, "lane_tile", "strand", (TL,),
   "const uint32_t inval = halo_lane ? 0xFFFFu : ((uint32_t)bw & 0xFFFFu);", "const uint32_t inval = halo_lane ? 0x7FFFu : ((uint32_t)bw & 0xFFFFu);",
   "the halo lanes emit the window ending at their byte 0")
_m("lane_tile_tail_keep15", TILE, "lane_tile", "strand", (MI, TL),
   "        en.bad |= keep >= 16 ? 0u", "        en.bad |= keep >= 15 ? 0u",
   "the padding byte behind a last line of 15 input bytes counts as input")
_m("lane_tile_rc_operands", TILE, "lane_tile", "strand", (TL,),
   "Q[1] = alignbit(en.rcode, r1, sh_r);", "Q[1] = alignbit(r1, en.rcode, sh_r);",
   "the reverse-complement stream takes its words in the wrong order")
_m("lane_tile_fix_d15", TILE, "lane_tile", "strand", (TL,),
   "constexpr int D = FIX ? KFIX - 16 : 0, S = FIX ? 64 - 2 * KFIX : 0;", "constexpr int D = FIX ? KFIX - 15 : 0, S = FIX ? 64 - 2 * KFIX : 0;",
   "the k-specialised builds take the high word from one position off")
_m("sv2_lo_word_minus1", TILE, "lane_tile_sv2", "strand", (TL, XS),
   "fl[i] = fw[D + j];                                  // lo words", "fl[i] = fw[D + j - 1];                                  // lo words",
   "the forward low word ends one base early")
_m("sv2_light_min_pos3", TILE, "lane_tile_sv2", "strand", (TL, XS),
   "mp.pk_min16_crossed(fw[pos[0]], rw[D + pos[2]]),", "mp.pk_min16_crossed(fw[pos[0]], rw[D + pos[3]]),",
   "the histogram prefix of positions jp and jp + 8 takes a neighbour's reverse-complement half")
_m("sv2w_lazy_k_and_2", TILE, "lane_tile_sv2w", "strand", (TL, XS),
   "constexpr bool LAZY = (K & 1) && !FWD;", "constexpr bool LAZY = (K & 2) && !FWD;",
   "even k compare their candidates with the bits below the value in place")
_m("sv2_fwd_import_minus1", TILE, "lane_tile_sv2_fwd", "strand", (TL, XS),
   "for (int g = 2; g <= D; g++) fw[D - g] = xl.prev(kSlotFw + 16 - g, fw[D + 16 - g]);", "for (int g = 2; g <= D; g++) fw[D - g] = xl.prev(kSlotFw + 16 - g, fw[D + 15 - g]);",
   "the previous lane hands over the word one base early")
_m("sv2_fwd_light_pair", TILE, "lane_tile_sv2_fwd", "strand", (TL, XS),
   "T[i] = LIGHT ? fw[pos[i & 1]] : fw[pos[i]];", "T[i] = LIGHT ? fw[pos[i & 2]] : fw[pos[i]];",
   "the light build reads the histogram prefix of the wrong position pair")
_m("sv2_light_34", TILE, "Sv2Light", "strand", (TL, XS),
   "static constexpr bool value = K >= 17 && 2 * K - HB <= 32; };", "static constexpr bool value = K >= 17 && 2 * K - HB <= 34; };",
   "k = 24 with 14-bit cells rebuilds its digests from a low word that lacks two bits")

# ---- minimizers --------------------------------------------------------------------------------------------------------------------------
_m("keyg_prev_strand_not_imported", TILE, "key_prev", "minimizer", (TL, MS),
   "r.s = xl.prev_auto(v.s);", "r.s = v.s;",
   "an imported key carries the strand of this lane's k-mer")
_m("min_shifted_tie_swapped", TILE, "min_shifted", "minimizer", (TL, MS),
   "X[j] = key_min(j >= Q ? Y[j - Q] : imp[j], X[j]);", "X[j] = key_min(X[j], j >= Q ? Y[j - Q] : imp[j]);",
   "the younger operand comes first: ties go to the rightmost k-mer (general keys)")
_m("min_shifted16_tie_swapped", TILE, "min_shifted", "minimizer", (TL, MS),
   "X[8 * h + j] = key_min(imp[j], X[8 * h + j]);", "X[8 * h + j] = key_min(X[8 * h + j], imp[j]);",
   "w >= 32, general keys: the round over 16 positions prefers the younger half")
_m("min_overlap_double_hop", TILE, "min_overlap", "minimizer", (TL, MS),
   "imp[j] = (j - S + 16 >= 0) ? key_prev", "imp[j] = (j - S + 16 > 0) ? key_prev",
   "overlap 16: position 0 hops two lanes back")
_m("min_invalid_tail_keep15", TILE, "minimizer_invalid16", "minimizer", (MI, TL, MS),
   "        bad |= keep >= 16 ? 0u", "        bad |= keep >= 15 ? 0u",
   "the padding byte behind a last line of 15 input bytes counts as input")
_m("min_invalid_smear_polarity", TILE, "minimizer_invalid16", "minimizer", (TL, MS),
   "const bool one_smear = a.min_smear_kw[0] != 0;", "const bool one_smear = a.min_smear_kw[0] == 0;",
   "spans beyond 49 take the one-smear table, which is all zero for them")
_m("keys_f64_tag_strand", TILE, "minimizer_keys_f64", "minimizer", (TL, MS),
   "tagR = (lane << 5) | fbitR;", "tagR = (lane << 5) | fbitF;",
   "both strands carry the same strand bit")
_m("keys_f64_tag_lane4", TILE, "minimizer_keys_f64", "minimizer", (TL, MS),
   "const uint32_t tagF = (lane << 5) | fbitF,", "const uint32_t tagF = (lane << 4) | fbitF,",
   "forward keys of neighbouring lanes share their position tags")
_m("keys_general_tie", TILE, "minimizer_keys_general", "minimizer", (TL, MS, MI),
   "const bool take_rc = TIE_RC ? (r <= f) : (r < f);", "const bool take_rc = TIE_RC ? (r < f) : (r < f);",
   "byte path: a k-mer equal to its reverse complement reports forward")
_m("van_herk_h_gt_2", TILE, "min_van_herk", "minimizer", (TL, MS),
   "if (H > 1) l = key_min(l, Fa);", "if (H > 2) l = key_min(l, Fa);",
   "w = 33 .. 48: the whole lane in the middle of the window is left out")
_m("slide_round16_from_33", TILE, "minimizer_slide", "minimizer", (TL, MS),
   "if (!kVanHerk && W >= 32) min_shifted<16>(xl, M, M);", "if (!kVanHerk && W >= 33) min_shifted<16>(xl, M, M);",
   "w = 32 with general keys stops at a span of 16")
_m("slide_van_herk_h", TILE, "minimizer_slide", "minimizer", (TL, MS),
   "const uint32_t H = (W - 1) >> 4;", "const uint32_t H = (W - 2) >> 4;",
   "w = 17 + 16 n counts one whole lane too few")
_m("set_window_q_lt", TILE, "scan_args_set_window", "minimizer", (TL, MS),
   "while (2 * q <= w) q *= 2;", "while (2 * q < w) q *= 2;",
   "w a power of two is made of two overlapping halves: w = 16 has no such form for the f64 keys")
_m("set_window_one_smear_50", TILE, "scan_args_set_window", "minimizer", (TL, MS, MI),
   "const uint32_t sft = kw <= 49 && len < kw", "const uint32_t sft = kw <= 50 && len < kw",
   "k + w - 1 = 50 takes the one-smear form, whose 64 bits hold only 48 earlier positions")
_m("sv2_min_a0_16", TILE, "lane_tile_sv2_min", "minimizer", (TL, MS),
   "constexpr int A0 = 17 - W;", "constexpr int A0 = 16 - W;",
   "windows reaching into the previous lane hold one k-mer too many")
_m("sv2_min_import_index_30", TILE, "lane_tile_sv2_min", "minimizer", (TL, MS),
   "xl.prev_add(kSlotSufLo + a, (uint32_t)suf[a], 0u - 32u);       // low word: index -= 16", "xl.prev_add(kSlotSufLo + a, (uint32_t)suf[a], 0u - 30u);       // low word: index -= 16",
   "the previous lane's last key shares its index with own position 0: a tie between them goes by the strand bit")

# ---- k = 33 .. 255 -----------------------------------------------------------------------------------------------------------------------
_m("wk_stage_tail_keep15", TILE, "wk_stage_slot", "wide", (MI, TL, WS),
   "else if (keep < 16) r.bad |= 0xFFFFu >> (uint32_t)keep;", "else if (keep < 15) r.bad |= 0xFFFFu >> (uint32_t)keep;",
   "the padding byte behind a last line of 15 input bytes counts as input")
_m("wk_valid16_own_15", TILE, "wk_valid16", "wide", (TL, WS),
   "((0xFFFFu << (16u - first_bad)) & 0xFFFFu);", "((0xFFFFu << (15u - first_bad)) & 0xFFFFu);",
   "the window ending on the slot's own first break is emitted")
_m("wk_back_words_14", TILE, "wk_back_words", "wide", (TL, WS),
   "return (k - 1u + 15u) >> 4; }", "return (k - 1u + 14u) >> 4; }",
   "k = 2 mod 16 starts its window one word late")
_m("wk_base_bits_k2", TILE, "wk_base_bits", "wide", (TL, WS),
   "return 2u * ((16u - ((k - 1u) & 15u)) & 15u); }", "return 2u * ((16u - ((k - 2u) & 15u)) & 15u); }",
   "the first window starts one base late")
_m("wk_strand_rc_operands", TILE, "wk_strand", "wide", (TL, WS),
   "V1 = J < 15 ? alignbit(w.rc0, w.rc1, 2 * J + 2) : w.rc0;", "V1 = J < 15 ? alignbit(w.rc1, w.rc0, 2 * J + 2) : w.rc0;",
   "the reverse complement's first 16 bases take their words in the wrong order")
_m("wk_strand_top_swapped", TILE, "wk_strand", "wide", (TL, WS),
   "top = lt ? F1 : V1;", "top = lt ? V1 : F1;",
   "the histogram bin comes from the strand that lost")

# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------------
_m("plan_tile_count_plus1", PLAN, "tile_count", "host", (XS,),
   "return (n + stride - 1) / stride; }", "return (n + stride) / stride; }",
   "an input of whole tiles gets an empty tile more")
_m("plan_first_tail", PLAN, "plan_launch", "host", (XS,),
   "const uint64_t first_tail = n / stride;", "const uint64_t first_tail = (n + 1) / stride;",
   "a tile whose last byte is the input's last but one is no tail tile")
_m("plan_tiles_per_shard", PLAN, "plan_launch", "host", (XS,),
   "p.tiles_per_shard = (uint32_t)((tiles + p.n_shards - 1) / p.n_shards);", "p.tiles_per_shard = (uint32_t)((tiles + p.n_shards) / p.n_shards);",
   "shards that divide the tiles evenly get one tile more each")
_m("plan_max_tiles_21", PLAN, "kMaxTilesPerLaunch", "host", (XS,),
   "constexpr uint64_t kMaxTilesPerLaunch = (uint64_t)8 << 22;", "constexpr uint64_t kMaxTilesPerLaunch = (uint64_t)8 << 21;",
   "launches of half the size")
_m("chunks_halo_14", CHUNKS, "chunk_halo", "host", (CH,),
   "return ((uint64_t)k - 1 + 15) & ~(uint64_t)15; }", "return ((uint64_t)k - 1 + 14) & ~(uint64_t)15; }",
   "k = 2 mod 16 gets a halo shorter than k - 1")
_m("chunks_halo_added", CHUNKS, "chunk_at", "host", (CH,),
   "start ? start - chunk_halo(k) : 0};", "start ? start + chunk_halo(k) : 0};",
   "a later chunk is materialised from behind its start")
_m("compat_cut_lt", COMPAT, "compat_cut", "host", (CP,),
   "per_record * (r1 + 1 - r0) <= chunk_bytes) r1++;", "per_record * (r1 + 1 - r0) < chunk_bytes) r1++;",
   "a record that fills the chunk exactly is left to the next one")
_m("trim_word_runs_ge", TRIM, "rt_word_runs", "host", (TR,),
   "if (run > r.best) { r.best = run; r.best_pos = at; }", "if (run >= r.best) { r.best = run; r.best_pos = at; }",
   "the rightmost of equal runs inside a word")
_m("trim_combine_mid_ge", TRIM, "rt_combine", "host", (TR,),
   "if (mid > r.best) { r.best = mid;", "if (mid >= r.best) { r.best = mid;",
   "a run across the seam wins a tie against an earlier run of the same length")

MUTANTS = tuple(_M)
BY_ID = {m.id: m for m in MUTANTS}

# three mutants whose kill is fast and recorded (the first audit's): tests/test_tile_mutants.py builds and runs them in parallel.
# (id, the test that must fail)
PINNED = (
    ("or_bytes_nb_gt4", "tests/test_quality_watch.py::test_quality_break_and_masked_watch_on_every_pair"),
    ("chunks_halo_14", "tests/test_chunks.py::test_chunks_tile_the_batch_with_whole_windows"),
    ("wk_valid16_thr_minus1", "tests/test_tile_logic_emu.py::test_emu_wide_k_reduce"),
)

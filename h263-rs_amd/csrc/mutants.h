// mutants.h -- the ARITHMETIC MUTANTS of the kernels, all in one place (tests/test_gpu_mutation.py; never the product).
//
// A mutant build differs from the product in exactly one arithmetic detail that the reference fixes bit for bit.  The
// parity suite is run against each of them on the MI355X and must fail where a soft-float model of the mutation says it
// will: that is the evidence that "bit-exact" in those tests means something.  The product build defines none of the
// macros below; every switch is then a compile-time `false` and the kernels contain nothing of this file.
//   -DH263MI_MUTATE_PAIRWISE             idct_1d sums its eight products as a balanced tree (idct.rs:52-65 sums in order)
//   -DH263MI_MUTATE_DEQUANT_SATURATION   the dequantiser's saturated values keep their low bits: 2047.9375 instead of 2047
//   -DH263MI_MUTATE_DEQUANT_WRAP         the dequantiser of wide LEVELs saturates where the reference's i16 product wraps
//   (the fourth mutant, libh263mi_fma.so, is a compiler flag: -ffp-contract=fast fuses the IDCT's multiplies into its adds)
// ... and two of the motion compensation (tests/test_gpu_mutation.py with tests/mc_mutation_probe.py):
//   -DH263MI_MUTATE_BLEND_ROUNDING       blend_rows adds its extra one wherever both dropped bits are set, also where an odd
//                                        Ha + Hb has absorbed it: +1 in some pixels of (1/2, 1/2) pieces, nowhere else
//   -DH263MI_MUTATE_INTEGER_BORDER       border lanes of a wave whose vectors are all integer skip the clamped re-gather and
//                                        use the bytes of their window as loaded
// ... and three of the deblocking post-filter (tests/test_gpu_mutation.py with tests/post_mutation_probe.py):
//   -DH263MI_MUTATE_DEBLOCK_HALF_ROUNDING    quartet_consts sets c1 = 0: |d1 / 2| rounds toward zero also where the reference
//                                            shifts a negative d1 (deblock.rs:109): A and D off by one where that limit clips
//   -DH263MI_MUTATE_DEBLOCK_FLOOR_EVERYWHERE trunc_mask is always 0: the scalar tails of the reference (deblock.rs:34-36) divide
//                                            with shifts like its SIMD lanes
//   -DH263MI_MUTATE_DEBLOCK_WRAP_COLUMNS     post_phase_hedges hands hfilter2 the strip column, not the picture column: the
//                                            columns that ride in the last tile (post_tile_columns) miss the horizontal edges
// ... and three of the reconstruction waves' bookkeeping (tests/test_gpu_mutation.py with tests/wave_mutation_probe.py):
//   -DH263MI_MUTATE_KILL_IGNORED             recon_phase_mark takes `killed` as 0: a coded block whose run walked past position
//                                            63 (rle.rs:125-127) goes through the IDCT with the LEVELs of its pool slot
//   -DH263MI_MUTATE_STATIC_IGNORES_MOTION    recon_wave_is_static ignores any_moving: eight uncoded inter macroblocks are
//                                            copied from the reference whatever their vectors are
//   -DH263MI_MUTATE_UNCODED_INTRA_DC         recon_phase_mark takes dc_nonzero as 0: an uncoded block of an intra macroblock
//                                            is never activated and stays at zero (the Dc class of rle.rs:151-160 is lost)
// ... and two of the bilinear / bicubic resampling (filter_kernel.inl), which the CPU checker alone is built with
// (tests/test_sim_filter.py):
//   -DH263MI_MUTATE_FILTER_SINGLE_ROUNDING   the horizontal pass hands on its unrounded sum: one weighted sum, one rounding
//   -DH263MI_MUTATE_FILTER_NO_CLAMP          the horizontal pass keeps the low 8 bits of a value outside 0..255 instead of
//                                            clamping it
// ... and two of the change maps (change_kernel.inl), which the CPU checker alone is built with (tests/test_sim_change.py):
//   -DH263MI_MUTATE_CHANGE_EDGE_AS_FULL      change_judge compares an edge cell as if it were full: the raw SAD against the
//                                            threshold instead of the mean difference
//   -DH263MI_MUTATE_CHANGE_SEGMENT_CELL      change_item takes a later segment's first cell from the pixel in front of the
//                                            segment: its first chunk (and every one behind it) is attributed to the cell on
//                                            its left
// ... and two of the plane histograms (hist_kernel.inl), which the CPU checker alone is built with (tests/test_sim_hist.py):
//   -DH263MI_MUTATE_HIST_CUT_CHUNK_FULL      hist_count takes a chunk that the picture's right edge cuts short as a whole one: the
//                                            missing pixels are counted as zeros
//   -DH263MI_MUTATE_HIST_PERCENTILE_STRICT   hist_reached compares 1000 * C(v) > q * P where the contract says >=: a percentile
//                                            that is reached exactly moves to the next value with a count
// ... and two of the motion regions (regions_kernel.inl), which the CPU checker alone is built with (tests/test_sim_regions.py):
//   -DH263MI_MUTATE_REGIONS_DIAGONAL         under connectivity 8 a cell is not joined with its down-left neighbour (the cell below
//                                            never looks up and to the right)
//   -DH263MI_MUTATE_REGIONS_BOX_CLIP         a box's right and bottom edges are not clipped to W and H: a box that holds partial
//                                            edge cells reaches behind the picture
// ... and three of the region tracks (tracks_kernel.inl), which the CPU checker alone is built with (tests/test_sim_tracks.py):
//   -DH263MI_MUTATE_TRACKS_FLOAT_IOU         two pairs are compared by their float32 quotients inter / union, not by the cross
//                                            products in integers
//   -DH263MI_MUTATE_TRACKS_ARGMAX            one round only: every track takes its best eligible detection, chosen by another
//                                            track or not
//   -DH263MI_MUTATE_TRACKS_BIRTH_BEFORE_DEATH  the births do not see the slots that a cut or a death freed in the same call
// ... and two of the background model (background_kernel.inl), which the CPU checker alone is built with (tests/test_sim_bg.py):
//   -DH263MI_MUTATE_BG_STEP_FLOOR            bg_step is d >> shift alone: a word less than 2^shift below c << 7 never arrives
//   -DH263MI_MUTATE_BG_JUDGE_AFTER           a pixel is judged against its word after the background-rate update, not before
// Two parts.  The switches need nothing and are included by post_kernel.inl and recon_kernel.inl; the IDCT helper is included
// by recon_kernel.inl (which defines H263MI_MUTANTS_WITH_IDCT) behind the definitions it uses (f32x2, splat2, BasisPtr,
// basis_pair).
#ifndef H263MI_MUTANTS_SWITCHES_H
#define H263MI_MUTANTS_SWITCHES_H

namespace h263mi {
namespace mutants {

#if defined(H263MI_MUTATE_PAIRWISE)
constexpr bool kPairwise = true;
#else
constexpr bool kPairwise = false;
#endif
#if defined(H263MI_MUTATE_DEQUANT_SATURATION)
constexpr bool kDequantSaturation = true;
#else
constexpr bool kDequantSaturation = false;
#endif
#if defined(H263MI_MUTATE_DEQUANT_WRAP)
constexpr bool kDequantWrap = true;
#else
constexpr bool kDequantWrap = false;
#endif
#if defined(H263MI_MUTATE_BLEND_ROUNDING)
constexpr bool kBlendRounding = true;
#else
constexpr bool kBlendRounding = false;
#endif
#if defined(H263MI_MUTATE_INTEGER_BORDER)
constexpr bool kIntegerBorder = true;
#else
constexpr bool kIntegerBorder = false;
#endif
#if defined(H263MI_MUTATE_DEBLOCK_HALF_ROUNDING)
constexpr bool kDeblockHalfRounding = true;
#else
constexpr bool kDeblockHalfRounding = false;
#endif
#if defined(H263MI_MUTATE_DEBLOCK_FLOOR_EVERYWHERE)
constexpr bool kDeblockFloorEverywhere = true;
#else
constexpr bool kDeblockFloorEverywhere = false;
#endif
#if defined(H263MI_MUTATE_DEBLOCK_WRAP_COLUMNS)
constexpr bool kDeblockWrapColumns = true;
#else
constexpr bool kDeblockWrapColumns = false;
#endif
#if defined(H263MI_MUTATE_KILL_IGNORED)
constexpr bool kKillIgnored = true;
#else
constexpr bool kKillIgnored = false;
#endif
#if defined(H263MI_MUTATE_STATIC_IGNORES_MOTION)
constexpr bool kStaticIgnoresMotion = true;
#else
constexpr bool kStaticIgnoresMotion = false;
#endif
#if defined(H263MI_MUTATE_UNCODED_INTRA_DC)
constexpr bool kUncodedIntraDc = true;
#else
constexpr bool kUncodedIntraDc = false;
#endif
#if defined(H263MI_MUTATE_FILTER_SINGLE_ROUNDING)
constexpr bool kFilterSingleRounding = true;
#else
constexpr bool kFilterSingleRounding = false;
#endif
#if defined(H263MI_MUTATE_FILTER_NO_CLAMP)
constexpr bool kFilterNoClamp = true;
#else
constexpr bool kFilterNoClamp = false;
#endif
#if defined(H263MI_MUTATE_CHANGE_EDGE_AS_FULL)
constexpr bool kChangeEdgeAsFull = true;
#else
constexpr bool kChangeEdgeAsFull = false;
#endif
#if defined(H263MI_MUTATE_CHANGE_SEGMENT_CELL)
constexpr bool kChangeSegmentCell = true;
#else
constexpr bool kChangeSegmentCell = false;
#endif
#if defined(H263MI_MUTATE_HIST_CUT_CHUNK_FULL)
constexpr bool kHistCutChunkFull = true;
#else
constexpr bool kHistCutChunkFull = false;
#endif
#if defined(H263MI_MUTATE_HIST_PERCENTILE_STRICT)
constexpr bool kHistPercentileStrict = true;
#else
constexpr bool kHistPercentileStrict = false;
#endif
#if defined(H263MI_MUTATE_REGIONS_DIAGONAL)
constexpr bool kRegionsDiagonal = true;
#else
constexpr bool kRegionsDiagonal = false;
#endif
#if defined(H263MI_MUTATE_REGIONS_BOX_CLIP)
constexpr bool kRegionsBoxClip = true;
#else
constexpr bool kRegionsBoxClip = false;
#endif
#if defined(H263MI_MUTATE_TRACKS_FLOAT_IOU)
constexpr bool kTracksFloatIou = true;
#else
constexpr bool kTracksFloatIou = false;
#endif
#if defined(H263MI_MUTATE_TRACKS_ARGMAX)
constexpr bool kTracksArgmax = true;
#else
constexpr bool kTracksArgmax = false;
#endif
#if defined(H263MI_MUTATE_TRACKS_BIRTH_BEFORE_DEATH)
constexpr bool kTracksBirthBeforeDeath = true;
#else
constexpr bool kTracksBirthBeforeDeath = false;
#endif
#if defined(H263MI_MUTATE_BG_STEP_FLOOR)
constexpr bool kBgStepFloor = true;
#else
constexpr bool kBgStepFloor = false;
#endif
#if defined(H263MI_MUTATE_BG_JUDGE_AFTER)
constexpr bool kBgJudgeAfter = true;
#else
constexpr bool kBgJudgeAfter = false;
#endif

}  // namespace mutants
}  // namespace h263mi
#endif  // H263MI_MUTANTS_SWITCHES_H

#if defined(H263MI_MUTANTS_WITH_IDCT) && !defined(H263MI_MUTANTS_IDCT_H)
#define H263MI_MUTANTS_IDCT_H
namespace h263mi {
namespace mutants {

// kPairwise: the eight rounded products summed as a balanced tree instead of in the order of the frequency index
H263_DEV void idct_1d_pairwise(BasisPtr B, const float in[8], f32x2 out[4], f32x2 first)
{
#pragma unroll
    for (int ip = 0; ip < 4; ip++) {
        f32x2 pr[8];
        pr[0] = first;
#pragma unroll
        for (int f = 1; f < 8; f++) pr[f] = splat2(in[f]) * basis_pair(B, f, ip);
        out[ip] = ((pr[0] + pr[1]) + (pr[2] + pr[3])) + ((pr[4] + pr[5]) + (pr[6] + pr[7]));
    }
}

}  // namespace mutants
}  // namespace h263mi
#endif  // H263MI_MUTANTS_WITH_IDCT

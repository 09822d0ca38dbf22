// pfb_bank_cut.h -- how one call of a two-pass filterbank plan (pfb_bank.hip, route 0) divides its units into passes through the plan's
// scratch.  Pure host arithmetic, shared with tests/emu and the banks' emulators so that the cut that ships is the cut the CPU tests check.
//
// Unit u of the output needs the `window` input elements that start at u * hop and gives `unit_out` output elements.  A pass of n units
// puts n + min_rows - 1 rows of `row` cf32 into the scratch: what the filter pass of n units reads (min_rows - 1 rows of history behind a
// transform that runs first; the unit's own row alone in front of a transform that runs second), so consecutive passes share input,
// never scratch.
//     synthesis bank              window = M P   hop = M   unit_out = M   min_rows = P   (unit: 1 output row)
//     oversampled channelizer     window = M P   hop = H   unit_out = M   min_rows = 1   (unit: 1 row)
//     oversampled synthesis bank  window = M L   hop = M   unit_out = H   min_rows = L = ceil(M P / H)   (unit: 1 hop)
#pragma once
#include <stddef.h>

namespace redio {

struct BankCut { size_t window, hop, unit_out, min_rows, row; };
struct BankPass { size_t first, units, in_off, rows, out_off; }; // first unit, unit count, input offset, scratch rows, output offset

// the three families' cuts for M channels, P taps per branch and hop H (the table above); one signature, so that a create entry names its own
inline BankCut bank_cut_synth(size_t M, size_t P, size_t) { return {M * P, M, M, P, M}; }
inline BankCut bank_cut_os(size_t M, size_t P, size_t H) { return {M * P, H, M, 1, M}; }
inline BankCut bank_cut_os_synth(size_t M, size_t P, size_t H)
{
    const size_t L = (M * P + H - 1) / H; // pfboss_L
    return {M * L, M, H, L, M};
}

inline size_t bank_units(const BankCut &c, size_t n_in) { return n_in < c.window ? 0 : (n_in - c.window) / c.hop + 1; }
// what a call of `units` units reads
inline size_t bank_input(const BankCut &c, size_t units) { return (units - 1) * c.hop + c.window; }

// the plan's chunk_rows from what set_chunk_rows was given: 0 is the default, 64 MiB of rows; fewer than min_rows count as min_rows
inline size_t bank_chunk_rows(const BankCut &c, size_t asked)
{
    const size_t rows = asked ? asked : ((size_t)64 << 20) / (c.row * 8);
    return rows < c.min_rows ? c.min_rows : rows;
}

// scratch rows of the largest pass of a call of `units` units: what reserve sizes the scratch and the transform for
inline size_t bank_pass_rows(const BankCut &c, size_t chunk_rows, size_t units)
{
    const size_t all = units + c.min_rows - 1;
    return all < chunk_rows ? all : chunk_rows;
}
inline size_t bank_passes(const BankCut &c, size_t chunk_rows, size_t units)
{
    const size_t per = bank_pass_rows(c, chunk_rows, units) - c.min_rows + 1;
    return (units + per - 1) / per;
}
inline BankPass bank_pass(const BankCut &c, size_t chunk_rows, size_t units, size_t i)
{
    const size_t per = bank_pass_rows(c, chunk_rows, units) - c.min_rows + 1, first = i * per;
    const size_t n = units - first < per ? units - first : per;
    return {first, n, first * c.hop, n + c.min_rows - 1, first * c.unit_out};
}

} // namespace redio

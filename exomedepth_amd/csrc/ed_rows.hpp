// ed_rows.hpp -- a row of exons against the plan's design: the one check behind every entry that takes regions or call rows.  Host-only:
// no HIP, no device types; tools/ratio_plan_check.cpp and tools/power_plan_check.cpp check it stand-alone.
#pragma once
#include <cstdint>

namespace edrows {
// a region (chromosome, first exon, last exon; global exon indices): 0 fine, 1 first > last, 2 chromosome out of range, 3 not inside its
// chromosome (an exon outside the plan, or a run that crosses a chromosome boundary)
inline int row_fault(int32_t chrom, int32_t first, int32_t last, int32_t C, const int32_t* chrom_off)
{
  if (chrom < 0 || chrom >= C) return 2;
  if (first > last) return 1;
  if (first < chrom_off[chrom] || last >= chrom_off[chrom + 1]) return 3;
  return 0;
}
// a call row, a region of one sample: 4 sample out of range, else the region's code
inline int row_fault(int32_t sample, int32_t chrom, int32_t first, int32_t last, int64_t n_samples, int32_t C, const int32_t* chrom_off)
{
  if (sample < 0 || sample >= n_samples) return 4;
  return row_fault(chrom, first, last, C, chrom_off);
}
}  // namespace edrows

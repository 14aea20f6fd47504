// film_rows.h -- the film rows a reconstruction filter reaches (the halo a partitioned film needs).
#pragma once

#include <cstdint>

namespace dcrt {

uint32_t FilterSupportRows(float r, uint32_t H);

}  // namespace dcrt

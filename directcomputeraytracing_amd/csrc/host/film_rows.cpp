#include "film_rows.h"

#include <algorithm>
#include <cmath>

namespace dcrt {

// Rows beyond its own that a film row's SampleConvolution window reaches
// (SampleConvolution.hlsl:77-81), with the kernel's float arithmetic
// (film_pixel_window): floor(r + 0.5) in exact arithmetic, one more where py + 0.5 + r
// rounds up to the next integer (r just below k + 0.5).
uint32_t FilterSupportRows(float r, uint32_t H)
{
    if (!(r < (float)H)) return H;
    uint32_t rows = 0;
    for (uint32_t py = 0; py < H; ++py) {
        const float cy = (float)py + 0.5f;
        int ys = (int)std::floor(cy - r), ye = (int)std::floor(cy + r);
        ys = std::max(ys, 0);
        ye = std::min(ye, (int)H - 1);
        rows = std::max<uint32_t>(rows, (uint32_t)std::max(ye - (int)py, (int)py - ys));
    }
    return rows;
}

}  // namespace dcrt

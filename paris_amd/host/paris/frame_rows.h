// The rows of a band: which detector rows each pass of the driver's frame chain covers for the band a slab
// needs. Host only: no ctx, no device. tests/chain_rule.py restates the rule (band_rows) and tests/test_frame_rows_host.py holds
// this function to the restatement through demo/paris_hip_frame_rows.
#ifndef PARIS_AMD_HOST_FRAME_ROWS_H_
#define PARIS_AMD_HOST_FRAME_ROWS_H_

#include <algorithm>
#include <cstdint>
#include <string>

#include "types.h"

namespace paris
{
    namespace detail
    {
        inline void rt(int rc, const char* what)
        {
            if(rc != PARIS_HIP_SUCCESS)
                throw stage_runtime_error{std::string{what} + " failed: " + paris_hip_strerror(rc)};
        }

        struct row_range
        {
            std::uint32_t first = 0, count = 0;
        };

        struct frame_rows
        {
            row_range out;  // the band asked for: what the roll writes and everything after it -- weights, filter, backprojection -- reads
            row_range band; // the rows that are zinger-filtered, ring-corrected and linearised: `out`, with a roll the rows it reads for `out`
            row_range fix;  // the band widened by the zinger windows' one row: the rows whose defects are repaired
            row_range air;  // the band widened by that row plus the repair's reach: the rows the frame's air value is subtracted from
            row_range up;   // `air` hulled with the air rectangle's rows: the rows that are read, uploaded, binned and corrected
            row_range src;  // the source rows of `up`: bin_y times as many
        };

        // With a defect map the repair of a band's defects reads good pixels up to reach_rows rows beyond it (0 without a map): those
        // rows are read, uploaded and corrected as well, and nothing else is done to them. With --zingers the windows of the band's
        // pixels reach one row beyond it: the rows uploaded are the band widened by reach_rows + 1, the repair covers the band widened
        // by 1, so that a window on the band's edge sees the repaired pixels the whole-detector run sees, and the zinger filter covers
        // the band itself. With --air-region (air != nullptr) every frame's value comes from the rectangle's rows, whatever the band:
        // the rows uploaded become ONE range that holds the widened band and the rectangle's rows (the rows between them travel too:
        // a frame source reads one contiguous range), and the value is subtracted from the widened band. With a roll (roll != nullptr,
        // on det_geo) the band asked for is what the roll writes, and the rows every earlier pass covers start from the roll's source
        // range of it. Every widening is clipped to the detector's n_col rows; an empty band stays empty. Every slab's volume then
        // equals the whole-detector run's, bit for bit. (Zinger saturation is counted per band, against a max_hits made for the whole
        // detector: the slabs' volumes equal the whole-detector run's only while no frame saturates in either.)
        inline auto plan_frame_rows(row_range band, std::uint32_t n_col, std::uint32_t reach_rows, bool zingers, const paris_hip_air_region* air,
                                    std::uint32_t bin_y, const paris_hip_detector_roll* roll = nullptr, const detector_geometry* det_geo = nullptr)
            -> frame_rows
        {
            auto r = frame_rows{};
            r.out = band;
            if(roll != nullptr && band.count != 0)
                rt(paris_hip_detector_roll_source_rows(roll, det_geo, r.out.first, r.out.count, &band.first, &band.count), "detector_roll_source_rows()");
            r.band = r.fix = r.air = band;
            if(band.count != 0)
            {
                const auto widened = [&](std::uint32_t by) {
                    const auto first = band.first - std::min(band.first, by);
                    return row_range{first, std::min(n_col - (band.first + band.count), by) + band.first + band.count - first};
                };
                r.fix = widened(zingers ? 1u : 0u);
                r.air = widened(reach_rows + (zingers ? 1u : 0u));
            }
            r.up = r.air;
            if(band.count != 0 && air != nullptr)
            {
                r.up.first = std::min(r.air.first, air->y0);
                r.up.count = std::max(r.air.first + r.air.count, air->y0 + air->height) - r.up.first;
            }
            r.src = row_range{bin_y * r.up.first, bin_y * r.up.count};
            return r;
        }
    }
}

#endif

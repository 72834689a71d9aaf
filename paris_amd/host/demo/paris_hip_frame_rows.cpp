// The driver's row plan for a band (paris/frame_rows.h), case by case: what tests/test_frame_rows_host.py
// holds to the restatement in tests/chain_rule.py. Host only: no ctx is created, so it runs without a device.
//
// stdin, one case per line, 17 fields:
//   n_row n_col l_px_row l_px_col delta_s delta_t d_so d_od delta_phi   the detector (its n_col rows are what the plan clips to)
//   band_first band_count reach_rows zingers                            the band asked for, the repair's reach, 0 / 1
//   rect_y0 rect_height                                                 the air rectangle's rows; height 0: no rectangle
//   bin_y eta_deg                                                       the row bin factor; the roll in degrees, 0: no roll
// stdout, one line per case: first and count of out, band, fix, air, up and src. Exit code 1 on a line it cannot read or a plan
// that throws, with the line's number on stderr.
#include <cstdio>
#include <exception>

#include "paris/frame_rows.h"

int main()
{
    using namespace paris::detail;
    char line[512];
    for(unsigned long n = 1; std::fgets(line, sizeof line, stdin) != nullptr; ++n)
    {
        auto geo = paris::detector_geometry{};
        auto band = row_range{};
        auto rect = paris_hip_air_region{};
        unsigned reach = 0, zingers = 0, bin_y = 0;
        auto roll = paris_hip_detector_roll{};
        if(std::sscanf(line, "%u %u %f %f %f %f %f %f %f %u %u %u %u %u %u %u %f", &geo.n_row, &geo.n_col, &geo.l_px_row, &geo.l_px_col, &geo.delta_s,
                       &geo.delta_t, &geo.d_so, &geo.d_od, &geo.delta_phi, &band.first, &band.count, &reach, &zingers, &rect.y0, &rect.height, &bin_y,
                       &roll.eta_deg) != 17)
        {
            std::fprintf(stderr, "paris_hip_frame_rows: line %lu: cannot read 17 fields\n", n);
            return 1;
        }
        try
        {
            const auto r = plan_frame_rows(band, geo.n_col, reach, zingers != 0u, rect.height != 0u ? &rect : nullptr, bin_y,
                                           roll.eta_deg != 0.f ? &roll : nullptr, &geo);
            std::printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", r.out.first, r.out.count, r.band.first, r.band.count, r.fix.first, r.fix.count,
                        r.air.first, r.air.count, r.up.first, r.up.count, r.src.first, r.src.count);
        }
        catch(const std::exception& e)
        {
            std::fprintf(stderr, "paris_hip_frame_rows: line %lu: %s\n", n, e.what());
            return 1;
        }
    }
    return 0;
}

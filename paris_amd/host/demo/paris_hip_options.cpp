// The driver's option parsers (paris/options.h: the table of detail::find_option_parser), value by value: what tests/test_options_host.py holds to
// the expectations written into it. Host only: no ctx is created and no library function is called, so it runs without a device.
//
// stdin, one case per line: FLAG, one blank, VALUE -- everything after that blank up to the end of the line, blanks included; a
// line without a blank gives the empty value. Each case is parsed into a fresh program_options.
// stdout, one line per case: every field a parser can set as name=value, floats as %a; or `refused: <message>`.
#include <cstdio>
#include <cstring>
#include <string>

#include "paris/options.h"

namespace
{
    void print(const paris::program_options& po)
    {
        const auto u = [](const char* name, unsigned long v) { std::printf("%s=%lu ", name, v); };
        const auto i = [](const char* name, int v) { std::printf("%s=%d ", name, v); };
        const auto f = [](const char* name, double v) { std::printf("%s=%a ", name, v); };
        u("bin_x", po.bin_x), u("bin_y", po.bin_y);
        u("zingers", po.zingers), f("zinger_abs", po.zinger_abs), f("zinger_rel", po.zinger_rel), i("zinger_polarity", po.zinger_polarity);
        u("extend_rows", po.extend_rows), u("extend_taper", po.extend_taper), u("extend_edge", po.extend_edge);
        u("rings", po.rings), u("ring_half_width", po.ring_half_width), f("ring_floor", po.ring_floor), f("ring_limit", po.ring_limit);
        u("find_axis", po.find_axis), f("axis_lo", po.axis_lo), f("axis_hi", po.axis_hi), f("axis_step", po.axis_step);
        u("axis_rows", po.axis_rows), u("axis_rows_given", po.axis_rows_given);
        u("roll", po.roll), f("roll_deg", po.roll_deg);
        u("find_roll", po.find_roll), f("roll_lo", po.roll_lo), f("roll_hi", po.roll_hi), f("roll_step", po.roll_step);
        u("air", po.air), u("air_x0", po.air_region.x0), u("air_y0", po.air_region.y0), u("air_width", po.air_region.width);
        u("air_height", po.air_region.height), f("air_limit", po.air_region.limit_abs);
        u("phase", po.phase), u("phase_material", po.phase_material), f("phase_delta_beta", po.phase_delta_beta), f("phase_energy", po.phase_energy);
        u("phase_margin", po.phase_margin), f("phase_alpha", po.phase_setting.alpha_mm2);
        u("phase_floor_given", po.phase_floor_given), f("phase_floor", po.phase_setting.t_min);
        u("scatter", po.scatter), u("scatter_detail_given", po.scatter_detail_given), f("scatter_amplitude", po.scatter_setting.amplitude);
        f("scatter_alpha", po.scatter_setting.alpha), f("scatter_beta", po.scatter_setting.beta), f("scatter_sigma1", po.scatter_setting.sigma1_mm);
        f("scatter_sigma2", po.scatter_setting.sigma2_mm), f("scatter_weight2", po.scatter_setting.weight2), f("scatter_limit", po.scatter_setting.limit);
        u("scatter_iterations", po.scatter_setting.iterations), u("scatter_margin", po.scatter_setting.margin);
        u("starvation", po.starvation), f("starvation_p0", po.starvation_setting.p0), f("starvation_gain", po.starvation_setting.gain);
        u("starvation_radius", po.starvation_setting.radius);
        u("denoise", po.denoise), u("denoise_radius_given", po.denoise_radius_given), f("denoise_sigma_r", po.denoise_setting.sigma_r);
        f("denoise_sigma_s", po.denoise_setting.sigma_s), u("denoise_radius", po.denoise_setting.radius);
        u("beam_hardening", po.beam_hardening), u("fit_beam_hardening", po.fit_beam_hardening), u("bh_degree", po.bh.degree);
        for(int k = 0; k < 4; ++k)
            f(("bh_c" + std::to_string(k + 1)).c_str(), po.bh.c[k]);
        u("bh_slices", po.bh_slices), u("bh_margin", po.bh_margin);
        u("lag", po.lag), u("lag_terms", po.lag_model.terms);
        for(int k = 0; k < 4; ++k)
            f(("lag_b" + std::to_string(k + 1)).c_str(), po.lag_model.b[k]), f(("lag_a" + std::to_string(k + 1)).c_str(), po.lag_model.a[k]);
        u("lag_start_given", po.lag_start_given), i("lag_start", po.lag_model.start);
        u("metal", po.metal), f("metal_threshold", po.metal_threshold), u("metal_grow", po.metal_grow), f("metal_min_path", po.metal_min_path);
        i("voxel_type", po.voxels.type), u("voxel_range_given", po.voxels.range_given), u("voxel_automatic", po.voxels.automatic);
        f("voxel_lo", po.voxels.lo), f("voxel_hi", po.voxels.hi), f("voxel_p_lo", po.voxels.p_lo), f("voxel_p_hi", po.voxels.p_hi);
        std::printf("\n");
    }
}

int main()
{
    char line[1024];
    while(std::fgets(line, sizeof line, stdin) != nullptr)
    {
        line[std::strcspn(line, "\n")] = '\0';
        const auto blank = std::strchr(line, ' ');
        const auto flag = blank != nullptr ? std::string{line, blank} : std::string{line};
        const auto value = std::string{blank != nullptr ? blank + 1 : ""};
        try
        {
            const auto parse = paris::detail::find_option_parser(flag);
            if(parse == nullptr)
                throw paris::stage_construction_error{"unknown option " + flag};
            auto po = paris::program_options{};
            parse(value, po);
            print(po);
        }
        catch(const paris::stage_construction_error& e)
        {
            std::printf("refused: %s\n", e.what());
        }
    }
    return 0;
}

// A PARIS-style driver over the C++ backend mirror: the per-device loop of src/main.cpp:79-109 with the file
// stages replaced by raw float32 files, so tests can feed known projections and compare the volume.
//
// usage: paris_hip_demo <n_row> <n_col> <l_px_row> <l_px_col> <delta_s> <delta_t> <d_so> <d_od> <delta_phi>
//                       <n_proj> <in.raw | lcg> <out.raw> [--no-weight] [--no-filter]
//                       [--slabs N] [--roi x1 x2 y1 y2 z1 z2] [--vol dx dy dz l_vx] [--cycle K] [--no-out] [--order N] [--json]
//                       [--short-scan start_deg range_deg] [--offset-detector] [--flat dark.raw|none flat.raw t_min]
//                       [--reproject frames.raw] [--defects mask.raw] [--zingers abs rel polarity]
//                       [--rings half_width floor limit] [--find-axis lo step count rows]
//                       [--extend-rows W M] [--bin BX BY mask.raw|none] [--air-region x0 y0 width height limit] [--detector-roll deg]
//                       [--lag steady|rest B1:A1[:B2:A2[:B3:A3[:B4:A4]]]]
//                       [--beam-hardening C1:C2[:C3[:C4]]] [--scatter A alpha beta sigma1 sigma2 w2 limit iterations margin]
//                       [--phase-alpha mm2 t_min margin] [--metal-trace bits.raw n_views] [--metal-voxels index.raw value.raw]
//                       [--denoise sigma_r sigma_s radius] [--starvation p0 gain radius] [--clear-after K]
// in.raw holds n_proj frames of n_col x n_row float32; "lcg" generates the SURVEY.md 8c noise frames.
// --cycle K: only K distinct lcg frames are held in host memory and projection i is frame i mod K (throughput runs over a whole
// circle of large frames: 1440 frames of 2048^2 would be 23 GiB); --no-out: the volume is neither read back nor written to out.raw.
// --json: one more line, the same figures as a JSON object (bench.py's paris_loop leg reads it).
// --short-scan: the projections (angle i * delta_phi) form a short scan over [start_deg, start_deg + range_deg]: set_short_scan() before
// the loops, so that paris::weight() applies the Parker redundancy weight first.
// --offset-detector: the projections come from an offset detector over a full circle: set_offset_detector() before the loops, so
// that paris::weight() applies the offset-detector redundancy weight before the cosine weight.
// --flat: the frames are intensities; dark.raw and flat.raw hold one n_col x n_row float32 frame each ("none": a zero dark).
// set_flat_field() before the loops, so that paris::weight() turns each frame into line integrals first.
// --defects: mask.raw holds n_col x n_row bytes, nonzero = defective pixel. set_defect_map() before the loops, so that paris::weight()
// repairs each frame's defective pixels after the dark / flat correction and before the weights.
// --air-region: the rectangle of the (binned) frame that sees only air, and limit_abs (0: none). set_air_region() before the loops, with the
// mask of --defects if there is one, so that paris::weight() subtracts each frame's own flux drift after the dark / flat correction and
// before the repair; the counts of air_stats() are printed as "air: ..." after the loops.
// --zingers: threshold_abs, threshold_rel and the polarity (1 bright, -1 dark, 0 both) of the zinger rule. set_zinger_filter() before the
// loops, so that paris::weight() removes each frame's outlier pixels after the repair and before the weights.
// --rings: half_width, floor_abs and limit_abs of the ring rule. A pre-pass before the loops sums every frame (ring_profile_add()) and
// set_ring_correction() gets the rule's correction frame, so that paris::weight() subtracts it after the zinger filter.
// --find-axis: the first candidate, the step, the number of candidates [pixels of delta_s] and the rows of the axis search. The same
// pre-pass hands every frame to axis_search_add() as well (the frames are a full circle at equal steps); the estimate is printed as
// "axis: delta_s = ..." and replaces the geometry's delta_s in the loops. The volume grid stays the one of the geometry given.
// --extend-rows: the taper length W and the number of edge pixels M of the row extension for truncated projections.
// set_row_extension() before the loops, so that paris::filter() adds the extension's response at its store.
// --detector-roll: the detector's in-plane rotation in degrees. set_detector_roll() before the loops (with the binned geometry under
// --bin), so that paris::weight() resamples each frame after the beam-hardening correction and before every weight.
// --lag: the frames are counts of a detector with lag (needs --flat). set_lag_correction() before the loops; this loop knows where a
// scan begins, so each slab's pass over the frames opens a sequence for whole frames (lag_begin()), corrects every loaded (and binned)
// frame in time order before paris::weight() corrects it to line integrals (lag_correct()), and closes it (lag_end()). Refused with
// --rings and --find-axis, whose pre-pass here does not run it.
// --bin: the geometry on the command line is the SOURCE detector's and in.raw holds frames of that size; each loaded frame is binned
// into a buffer of the binned detector (set_binning() before the loops, bin_frame() after paris::load()) and everything downstream runs
// with binned_geometry(). mask.raw: n_col x n_row bytes at source size, nonzero = left out of its bin. --flat, --defects and the other
// settings take frames of the BINNED size. Refused together with --rings and --reproject.
// --beam-hardening: the coefficients c_1 ... c_N of the polynomial, as many as are typed (the library refuses more than four).
// set_beam_hardening() before the loops, so that paris::weight() linearises each frame after the phase retrieval and before the roll.
// --scatter: the nine fields of paris_hip_scatter_correction in their order. set_scatter_correction() before the loops, with the
// binned detector's size and pitches under --bin, so that paris::weight() removes each frame's scatter after the ring correction.
// --starvation: the three fields of paris_hip_starvation_filter in their order. set_starvation_filter() before the loops, with the
// binned detector's size under --bin, so that paris::weight() smooths each frame's starved pixels after the ring correction and before
// the scatter correction.
// --phase-alpha: alpha [mm^2], the floor of the transmission and the margin. set_phase_retrieval() before the loops (binned size and
// pitches under --bin), so that paris::weight() low-passes each frame's transmission after the scatter correction.
// --metal-trace: bits.raw holds the packed traces of n_views views, n_views x n_col x words uint64 with words = ceil(n_row / 64)
// (paris_hip_metal_trace_pack's layout); a file of another size is refused. set_metal_trace() before the loops, so that paris::weight()
// inpaints each frame with the trace of view p.idx after the roll and before the weights.
// --metal-voxels: index.raw holds uint64 and value.raw as many float32, the list of paris_hip_metal_collect. set_metal_voxels() before
// the loops; after each slab's projection loop and before its read-back metal_reinsert() puts the slab's part of the list back.
// --denoise: sigma_r, sigma_s and the radius of the bilateral filter. Needs --slabs 1: after the loop (and the reinsertion) the volume
// is filtered into a second device volume by two volume_bilateral() calls, slices [0, h) and [h, dim_z) with h = dim_z / 2, each with
// the whole volume as its source, and the filtered volume is what is written.
// --clear-after K: after projection K of each slab's loop the settings of --beam-hardening, --starvation, --scatter, --phase-alpha, --metal-trace and
// --metal-voxels are undone with their clear_*() calls, and set again at the top of the next slab: projections 0 .. K of every slab
// pass through them, the others do not. (With --metal-voxels the list is gone when the slab is finished, so metal_reinsert() refuses.)
// A setting the library refuses ends the run with status 1 and its message before out.raw is opened.
// --reproject: the reconstruction is forward-projected at every angle of the scan (backend::forward_project) and the n_proj float32
// frames are written to frames.raw. One slab's volume is alive at a time: after a slab's projection loop each view is loaded from the
// host copy of the frames so far, the slab's part is added (the first slab writes) and the view is copied back; slabs go in
// ascending order. Refused together with --roi (the forward projector has no ROI form).
// out.raw receives the whole (ROI) volume, slabs written at their slice offsets (fixing SURVEY.md Q4).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "paris/stages.h"

namespace
{
    void lcg_fill(float* p, std::size_t n, std::uint32_t idx)
    {
        std::uint32_t s = 12345u + idx;
        for(std::size_t i = 0; i < n; ++i)
        {
            s = s * 1664525u + 1013904223u;
            p[i] = static_cast<float>(s >> 8) / 16777216.f;
        }
    }

    // a whole raw file of T; n != 0: it must hold exactly n of them
    template <typename T>
    auto read_raw(const std::string& path, std::size_t n) -> std::vector<T>
    {
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if(f == nullptr)
            throw paris::stage_runtime_error{"cannot read " + path};
        std::fseek(f, 0, SEEK_END);
        const auto bytes = static_cast<std::size_t>(std::ftell(f));
        std::fseek(f, 0, SEEK_SET);
        auto v = std::vector<T>(bytes / sizeof(T));
        const bool ok = bytes % sizeof(T) == 0 && (n == 0 || v.size() == n) && std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
        std::fclose(f);
        if(!ok)
            throw paris::stage_runtime_error{"cannot read " + path + ": " + std::to_string(bytes) + " byte(s), " + std::to_string(n * sizeof(T)) + " expected"};
        return v;
    }
}

int main(int argc, char** argv)
{
    if(argc < 13)
    {
        std::fprintf(stderr, "usage: see the header of paris_hip_demo.cpp\n");
        return 2;
    }
    try
    {
        auto det = paris::detector_geometry{};
        det.n_row = static_cast<std::uint32_t>(std::atoi(argv[1]));
        det.n_col = static_cast<std::uint32_t>(std::atoi(argv[2]));
        det.l_px_row = std::strtof(argv[3], nullptr);
        det.l_px_col = std::strtof(argv[4], nullptr);
        det.delta_s = std::strtof(argv[5], nullptr);
        det.delta_t = std::strtof(argv[6], nullptr);
        det.d_so = std::strtof(argv[7], nullptr);
        det.d_od = std::strtof(argv[8], nullptr);
        det.delta_phi = std::strtof(argv[9], nullptr);
        const auto n_proj = static_cast<std::uint32_t>(std::atoi(argv[10]));
        const auto in_path = std::string{argv[11]};
        const auto out_path = std::string{argv[12]};

        bool do_weight = true, do_filter = true, enable_roi = false, write_out = true, json = false;
        int slabs = 1;
        std::uint32_t cycle = 0;
        bool short_scan = false;
        float scan_start = 0.f, scan_range = 0.f;
        bool offset_detector = false, offset_first = false; // offset_first: --offset-detector came before --short-scan (setter order)
        std::string dark_path, flat_path, reproject_path, defects_path;
        float t_min = 1e-5f;
        bool zingers = false;
        float zinger_abs = 0.f, zinger_rel = 0.f;
        int zinger_polarity = 1;
        bool air = false;
        std::uint32_t air_rect[4] = {0, 0, 0, 0};
        float air_limit = 0.f;
        bool rings = false;
        std::uint32_t ring_half_width = 0;
        float ring_floor = 0.f, ring_limit = 0.f;
        bool find_axis = false;
        auto axis = paris_hip_axis_search{};
        bool extend_rows = false;
        std::uint32_t extend_taper = 0, extend_edge = 0;
        bool detector_roll = false;
        float roll_deg = 0.f;
        bool lag = false;
        int lag_start = PARIS_HIP_LAG_START_STEADY;
        std::uint32_t lag_terms = 0;
        float lag_b[PARIS_HIP_LAG_TERMS_MAX] = {0.f, 0.f, 0.f, 0.f}, lag_a[PARIS_HIP_LAG_TERMS_MAX] = {0.f, 0.f, 0.f, 0.f};
        std::uint32_t bin_x = 1, bin_y = 1;
        std::string bin_mask_path;
        std::uint32_t bh_degree = 0;
        float bh_c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; // as many as are typed: the library judges the degree
        bool scatter = false;
        auto scatter_setting = paris_hip_scatter_correction{};
        bool starvation = false;
        auto starvation_setting = paris_hip_starvation_filter{};
        bool phase = false;
        float phase_alpha = 0.f, phase_t_min = 0.f;
        std::uint32_t phase_margin = 0;
        std::string trace_path, voxel_index_path, voxel_value_path;
        std::uint32_t trace_views = 0;
        bool denoise = false;
        float denoise_sigma_r = 0.f, denoise_sigma_s = 0.f;
        std::uint32_t denoise_radius = 0;
        long clear_after = -1;
        bool vol_given = false;
        int order = -1; // --order N: workgroup -> tile order of the backprojection kernels (A/B; -1 = the library's choice)
        auto roi = paris::region_of_interest{};
        auto vol_geo = paris::calculate_volume_geometry(det);
        for(int a = 13; a < argc; ++a)
        {
            if(!std::strcmp(argv[a], "--no-weight")) do_weight = false;
            else if(!std::strcmp(argv[a], "--no-filter")) do_filter = false;
            else if(!std::strcmp(argv[a], "--slabs") && a + 1 < argc) slabs = std::atoi(argv[++a]);
            else if(!std::strcmp(argv[a], "--cycle") && a + 1 < argc) cycle = static_cast<std::uint32_t>(std::atoi(argv[++a]));
            else if(!std::strcmp(argv[a], "--no-out")) write_out = false;
            else if(!std::strcmp(argv[a], "--json")) json = true;
            else if(!std::strcmp(argv[a], "--order") && a + 1 < argc) order = std::atoi(argv[++a]);
            else if(!std::strcmp(argv[a], "--short-scan") && a + 2 < argc)
            {
                short_scan = true;
                scan_start = std::strtof(argv[a + 1], nullptr);
                scan_range = std::strtof(argv[a + 2], nullptr);
                a += 2;
            }
            else if(!std::strcmp(argv[a], "--offset-detector"))
            {
                offset_detector = true;
                offset_first = !short_scan;
            }
            else if(!std::strcmp(argv[a], "--flat") && a + 3 < argc)
            {
                dark_path = argv[a + 1];
                flat_path = argv[a + 2];
                t_min = std::strtof(argv[a + 3], nullptr);
                a += 3;
            }
            else if(!std::strcmp(argv[a], "--reproject") && a + 1 < argc) reproject_path = argv[++a];
            else if(!std::strcmp(argv[a], "--defects") && a + 1 < argc) defects_path = argv[++a];
            else if(!std::strcmp(argv[a], "--zingers") && a + 3 < argc)
            {
                zingers = true;
                zinger_abs = std::strtof(argv[a + 1], nullptr);
                zinger_rel = std::strtof(argv[a + 2], nullptr);
                zinger_polarity = std::atoi(argv[a + 3]);
                a += 3;
            }
            else if(!std::strcmp(argv[a], "--air-region") && a + 5 < argc)
            {
                air = true;
                for(int k = 0; k < 4; ++k)
                    air_rect[k] = static_cast<std::uint32_t>(std::strtoul(argv[a + 1 + k], nullptr, 10));
                air_limit = std::strtof(argv[a + 5], nullptr);
                a += 5;
            }
            else if(!std::strcmp(argv[a], "--rings") && a + 3 < argc)
            {
                rings = true;
                ring_half_width = static_cast<std::uint32_t>(std::strtoul(argv[a + 1], nullptr, 10));
                ring_floor = std::strtof(argv[a + 2], nullptr);
                ring_limit = std::strtof(argv[a + 3], nullptr);
                a += 3;
            }
            else if(!std::strcmp(argv[a], "--find-axis") && a + 4 < argc)
            {
                find_axis = true;
                axis.lo = std::strtof(argv[a + 1], nullptr);
                axis.step = std::strtof(argv[a + 2], nullptr);
                axis.count = static_cast<std::uint32_t>(std::strtoul(argv[a + 3], nullptr, 10));
                axis.rows = static_cast<std::uint32_t>(std::strtoul(argv[a + 4], nullptr, 10));
                a += 4;
            }
            else if(!std::strcmp(argv[a], "--extend-rows") && a + 2 < argc)
            {
                extend_rows = true;
                extend_taper = static_cast<std::uint32_t>(std::strtoul(argv[a + 1], nullptr, 10));
                extend_edge = static_cast<std::uint32_t>(std::strtoul(argv[a + 2], nullptr, 10));
                a += 2;
            }
            else if(!std::strcmp(argv[a], "--detector-roll") && a + 1 < argc)
            {
                detector_roll = true;
                roll_deg = std::strtof(argv[a + 1], nullptr);
                a += 1;
            }
            else if(!std::strcmp(argv[a], "--lag") && a + 2 < argc)
            {
                lag = true;
                lag_start = !std::strcmp(argv[a + 1], "rest") ? PARIS_HIP_LAG_START_REST : PARIS_HIP_LAG_START_STEADY;
                const char* at = argv[a + 2];
                for(std::uint32_t k = 0; k < 2u * PARIS_HIP_LAG_TERMS_MAX && *at != '\0'; ++k)
                {
                    char* end = nullptr;
                    (k % 2u == 0u ? lag_b : lag_a)[k / 2u] = std::strtof(at, &end);
                    lag_terms = k / 2u + 1u;
                    at = *end == ':' ? end + 1 : end;
                    if(end == at)
                        break;
                }
                a += 2;
            }
            else if(!std::strcmp(argv[a], "--beam-hardening") && a + 1 < argc)
            {
                const char* at = argv[++a];
                for(bh_degree = 0; bh_degree < 8u && *at != '\0';)
                {
                    char* end = nullptr;
                    bh_c[bh_degree] = std::strtof(at, &end);
                    if(end == at)
                        break;
                    ++bh_degree;
                    at = *end == ':' ? end + 1 : end;
                }
            }
            else if(!std::strcmp(argv[a], "--scatter") && a + 9 < argc)
            {
                scatter = true;
                scatter_setting.amplitude = std::strtof(argv[a + 1], nullptr);
                scatter_setting.alpha = std::strtof(argv[a + 2], nullptr);
                scatter_setting.beta = std::strtof(argv[a + 3], nullptr);
                scatter_setting.sigma1_mm = std::strtof(argv[a + 4], nullptr);
                scatter_setting.sigma2_mm = std::strtof(argv[a + 5], nullptr);
                scatter_setting.weight2 = std::strtof(argv[a + 6], nullptr);
                scatter_setting.limit = std::strtof(argv[a + 7], nullptr);
                scatter_setting.iterations = static_cast<std::uint32_t>(std::strtoul(argv[a + 8], nullptr, 10));
                scatter_setting.margin = static_cast<std::uint32_t>(std::strtoul(argv[a + 9], nullptr, 10));
                a += 9;
            }
            else if(!std::strcmp(argv[a], "--phase-alpha") && a + 3 < argc)
            {
                phase = true;
                phase_alpha = std::strtof(argv[a + 1], nullptr);
                phase_t_min = std::strtof(argv[a + 2], nullptr);
                phase_margin = static_cast<std::uint32_t>(std::strtoul(argv[a + 3], nullptr, 10));
                a += 3;
            }
            else if(!std::strcmp(argv[a], "--metal-trace") && a + 2 < argc)
            {
                trace_path = argv[a + 1];
                trace_views = static_cast<std::uint32_t>(std::strtoul(argv[a + 2], nullptr, 10));
                a += 2;
            }
            else if(!std::strcmp(argv[a], "--metal-voxels") && a + 2 < argc)
            {
                voxel_index_path = argv[a + 1];
                voxel_value_path = argv[a + 2];
                a += 2;
            }
            else if(!std::strcmp(argv[a], "--denoise") && a + 3 < argc)
            {
                denoise = true;
                denoise_sigma_r = std::strtof(argv[a + 1], nullptr);
                denoise_sigma_s = std::strtof(argv[a + 2], nullptr);
                denoise_radius = static_cast<std::uint32_t>(std::strtoul(argv[a + 3], nullptr, 10));
                a += 3;
            }
            else if(!std::strcmp(argv[a], "--starvation") && a + 3 < argc)
            {
                starvation = true;
                starvation_setting.p0 = std::strtof(argv[a + 1], nullptr);
                starvation_setting.gain = std::strtof(argv[a + 2], nullptr);
                starvation_setting.radius = static_cast<std::uint32_t>(std::strtoul(argv[a + 3], nullptr, 10));
                a += 3;
            }
            else if(!std::strcmp(argv[a], "--clear-after") && a + 1 < argc) clear_after = std::atol(argv[++a]);
            else if(!std::strcmp(argv[a], "--bin") && a + 3 < argc)
            {
                bin_x = static_cast<std::uint32_t>(std::strtoul(argv[a + 1], nullptr, 10));
                bin_y = static_cast<std::uint32_t>(std::strtoul(argv[a + 2], nullptr, 10));
                bin_mask_path = argv[a + 3];
                a += 3;
            }
            else if(!std::strcmp(argv[a], "--roi") && a + 6 < argc)
            {
                enable_roi = true;
                roi.x1 = std::atoi(argv[a + 1]); roi.x2 = std::atoi(argv[a + 2]);
                roi.y1 = std::atoi(argv[a + 3]); roi.y2 = std::atoi(argv[a + 4]);
                roi.z1 = std::atoi(argv[a + 5]); roi.z2 = std::atoi(argv[a + 6]);
                a += 6;
            }
            else if(!std::strcmp(argv[a], "--vol") && a + 4 < argc)
            {
                vol_geo.dim_x = std::atoi(argv[a + 1]); vol_geo.dim_y = std::atoi(argv[a + 2]); vol_geo.dim_z = std::atoi(argv[a + 3]);
                vol_geo.l_vx_x = vol_geo.l_vx_y = vol_geo.l_vx_z = std::strtof(argv[a + 4], nullptr);
                vol_given = true;
                a += 4;
            }
            else
            {
                std::fprintf(stderr, "unknown argument %s\n", argv[a]);
                return 2;
            }
        }
        if(!reproject_path.empty() && enable_roi)
        {
            std::fprintf(stderr, "--reproject cannot be combined with --roi: the forward projector has no ROI form\n");
            return 2;
        }
        const bool binning = !bin_mask_path.empty();
        if(binning && (rings || find_axis || !reproject_path.empty()))
        {
            std::fprintf(stderr, "--bin cannot be combined with --rings, --find-axis or --reproject\n");
            return 2;
        }
        if(lag && (rings || find_axis))
        {
            std::fprintf(stderr, "--lag cannot be combined with --rings or --find-axis\n");
            return 2;
        }
        if(denoise && slabs != 1)
        {
            std::fprintf(stderr, "--denoise needs --slabs 1: the filter reads the whole volume\n");
            return 2;
        }
        const auto src_det = det; // the detector the frames of in.raw come from
        if(binning)
        {
            det = paris::backend::binned_geometry(bin_x, bin_y, src_det);
            if(!vol_given)
                vol_geo = paris::calculate_volume_geometry(det);
        }
        auto roi_geo = vol_geo;
        if(enable_roi)
            roi_geo = paris::apply_roi(vol_geo, roi.x1, roi.x2, roi.y1, roi.y2, roi.z1, roi.z2); // src/main.cpp:125-130

        auto devices = paris::backend::get_devices();
        if(devices.empty())
            throw paris::stage_construction_error{"no HIP device"};
        paris::backend::set_device(devices[0]); // src/main.cpp:87
        if(offset_detector && offset_first)
            paris::backend::set_offset_detector();
        if(short_scan)
            paris::backend::set_short_scan(scan_start, scan_range, false);
        if(offset_detector && !offset_first)
            paris::backend::set_offset_detector();
        if(!flat_path.empty())
        {
            const auto n = std::size_t{det.n_row} * det.n_col;
            auto read_frame = [n](const std::string& path) {
                auto v = std::vector<float>(n);
                std::FILE* f = std::fopen(path.c_str(), "rb");
                const bool ok = f != nullptr && std::fread(v.data(), sizeof(float), n, f) == n;
                if(f != nullptr)
                    std::fclose(f);
                if(!ok)
                    throw paris::stage_construction_error{"cannot read " + path};
                return v;
            };
            const auto flat = read_frame(flat_path);
            const auto dark = dark_path == "none" ? std::vector<float>{} : read_frame(dark_path);
            paris::backend::set_flat_field(dark.empty() ? nullptr : dark.data(), flat.data(), det.n_row, det.n_col, t_min);
        }
        auto defect_mask = std::vector<std::uint8_t>{}; // --defects: the air region leaves its pixels out as well
        if(!defects_path.empty())
        {
            const auto n = std::size_t{det.n_row} * det.n_col;
            auto& mask = defect_mask;
            mask.resize(n);
            std::FILE* f = std::fopen(defects_path.c_str(), "rb");
            const bool ok = f != nullptr && std::fread(mask.data(), 1u, n, f) == n;
            if(f != nullptr)
                std::fclose(f);
            if(!ok)
                throw paris::stage_construction_error{"cannot read " + defects_path};
            paris::backend::set_defect_map(mask.data(), det.n_row, det.n_col);
        }
        if(air)
            paris::backend::set_air_region(air_rect[0], air_rect[1], air_rect[2], air_rect[3], det.n_row, det.n_col, 0u, air_limit,
                                           defect_mask.empty() ? nullptr : defect_mask.data());
        if(binning)
        {
            const auto n = std::size_t{src_det.n_row} * src_det.n_col;
            auto mask = std::vector<std::uint8_t>{};
            if(bin_mask_path != "none")
            {
                mask.resize(n);
                std::FILE* f = std::fopen(bin_mask_path.c_str(), "rb");
                const bool ok = f != nullptr && std::fread(mask.data(), 1u, n, f) == n;
                if(f != nullptr)
                    std::fclose(f);
                if(!ok)
                    throw paris::stage_construction_error{"cannot read " + bin_mask_path};
            }
            paris::backend::set_binning(bin_x, bin_y, mask.empty() ? nullptr : mask.data(), src_det.n_row, src_det.n_col);
        }
        if(zingers)
            paris::backend::set_zinger_filter(zinger_abs, zinger_rel, zinger_polarity, det.n_row, det.n_col);
        if(extend_rows)
            paris::backend::set_row_extension(extend_edge, extend_taper);
        if(detector_roll)
            paris::backend::set_detector_roll(roll_deg, det);
        if(lag)
            paris::backend::set_lag_correction(lag_b, lag_a, lag_terms, lag_start);
        // the settings --clear-after undoes: set here, before out.raw is opened, and again at the top of every slab that follows a clear
        const auto metal_bits = trace_path.empty() ? std::vector<std::uint64_t>{}
                                                   : read_raw<std::uint64_t>(trace_path, std::size_t{trace_views} * det.n_col * ((det.n_row + 63u) / 64u));
        const auto voxel_index = voxel_index_path.empty() ? std::vector<std::uint64_t>{} : read_raw<std::uint64_t>(voxel_index_path, 0u);
        const auto voxel_value = voxel_value_path.empty() ? std::vector<float>{} : read_raw<float>(voxel_value_path, voxel_index.size());
        if(!voxel_value_path.empty() && voxel_value.size() != voxel_index.size()) // (an empty list: read_raw's n == 0 checks nothing)
            throw paris::stage_runtime_error{"cannot read " + voxel_value_path + ": not one value per index"};
        const auto set_cleared = [&]() {
            if(bh_degree != 0u)
                paris::backend::set_beam_hardening(bh_c, bh_degree, det.n_row, det.n_col);
            if(starvation)
                paris::backend::set_starvation_filter(starvation_setting, det.n_row, det.n_col);
            if(scatter)
                paris::backend::set_scatter_correction(scatter_setting, det.n_row, det.n_col, det.l_px_row, det.l_px_col);
            if(phase)
                paris::backend::set_phase_retrieval(phase_alpha, phase_t_min, phase_margin, det.n_row, det.n_col, det.l_px_row, det.l_px_col);
            if(!trace_path.empty())
                paris::backend::set_metal_trace(metal_bits.data(), trace_views, det.n_row, det.n_col);
            if(!voxel_index_path.empty())
                paris::backend::set_metal_voxels(voxel_index.data(), voxel_value.data(), voxel_index.size());
        };
        const auto clear_set = [&]() {
            if(bh_degree != 0u)
                paris::backend::clear_beam_hardening();
            if(starvation)
                paris::backend::clear_starvation_filter();
            if(scatter)
                paris::backend::clear_scatter_correction();
            if(phase)
                paris::backend::clear_phase_retrieval();
            if(!trace_path.empty())
                paris::backend::clear_metal_trace();
            if(!voxel_index_path.empty())
                paris::backend::clear_metal_voxels();
        };
        set_cleared();
        if(order >= 0)
            paris::backend::detail::runtime_check(paris_hip_set_backproject_order(paris::backend::current_ctx(), order, -1), "--order");

        // fixed slab count (the memory-driven count is backend::make_subvolume_information)
        auto info = paris::subvolume_info{};
        info.num = slabs < 1 ? 1 : slabs;
        info.geo = {roi_geo.dim_x, roi_geo.dim_y, roi_geo.dim_z / static_cast<std::uint32_t>(info.num),
                    roi_geo.dim_z % static_cast<std::uint32_t>(info.num)};

        // all frames in host memory (the reference re-reads them per task: src/main.cpp:93)
        const auto frame = std::size_t{src_det.n_row} * src_det.n_col;
        const auto n_held = (in_path == "lcg" && cycle != 0 && cycle < n_proj) ? cycle : n_proj;
        auto frames = std::vector<float>(frame * n_held);
        if(in_path == "lcg")
            for(std::uint32_t i = 0; i < n_held; ++i)
                lcg_fill(frames.data() + frame * i, frame, i);
        else
        {
            std::FILE* f = std::fopen(in_path.c_str(), "rb");
            if(f == nullptr || std::fread(frames.data(), sizeof(float), frames.size(), f) != frames.size())
                throw paris::stage_runtime_error{"cannot read " + in_path};
            std::fclose(f);
        }

        if(rings || find_axis) // the pre-pass: every frame through correction, repair and zinger filter into the profile and the search
        {
            if(rings)
                paris::backend::ring_profile_begin(det.n_row, det.n_col);
            if(find_axis)
                paris::backend::axis_search_begin(axis, det, n_proj);
            for(std::uint32_t i = 0; i < n_proj; ++i)
            {
                auto p = paris::backend::make_projection_host(det.n_row, det.n_col);
                std::memcpy(p.buf.get(), frames.data() + frame * (i % n_held), frame * sizeof(float));
                p.idx = i;
                auto d_p = paris::load(p);
                if(rings)
                    paris::ring_profile_add(d_p);
                if(find_axis && rings) // the chain has run
                    paris::backend::axis_search_add(d_p.buf.get(), d_p.buf.pitch(), d_p.dim_x, d_p.dim_y, i);
                else if(find_axis)
                    paris::axis_search_add(d_p, i);
            }
            if(rings)
            {
                auto c = std::vector<float>(frame);
                paris::backend::ring_profile_finish(ring_half_width, ring_floor, ring_limit, c.data());
                paris::backend::set_ring_correction(c.data(), det.n_row, det.n_col);
            }
            if(find_axis)
            {
                auto cost = std::vector<double>(axis.count);
                const auto found = paris::backend::axis_search_finish(cost.data());
                std::printf("axis: delta_s = %.9g (candidate %u of %u, J_min / J_median %.3g, at_edge %u)\n", static_cast<double>(found.delta_s), found.best,
                            axis.count, found.cost_median > 0.0 ? found.cost_min / found.cost_median : 0.0, found.at_edge);
                det.delta_s = found.delta_s;
            }
        }

        std::FILE* out = write_out ? std::fopen(out_path.c_str(), "wb") : nullptr;
        if(write_out && out == nullptr)
            throw paris::stage_runtime_error{"cannot open " + out_path};

        auto reprojected = std::vector<float>(reproject_path.empty() ? std::size_t{0} : frame * n_proj); // --reproject: the frames so far

        using clock = std::chrono::steady_clock;
        double split_s[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // make_projection_host, frame fill, load, weight, filter, backproject, free device, free host
        double fill_s = 0.0, tail_s = 0.0; // of loop_s: the host's own frame fill (memcpy into the pinned buffer), the wait for the GPU after the last call
        double loop_s = 0.0; // the per-projection loops only (volume allocation, read-back and file output are not the hot path)
        for(int id = 0; id < info.num; ++id) // one task per slab: src/task.cpp:38-48, src/main.cpp:89-108
        {
            const bool last = (info.num - id) <= 1;
            auto v = paris::make_volume(info.geo, last);
            const auto offset = static_cast<std::uint32_t>(id) * info.geo.dim_z;
            if(clear_after >= 0 && id > 0) // the slab before has cleared them
                set_cleared();
            const auto t_start = std::chrono::steady_clock::now();
            if(lag) // this pass over the scan is a sequence of its own, from frame 0
                paris::backend::lag_begin(det.n_row, det.n_col, 0u, det.n_col);
            for(std::uint32_t i = 0; i < n_proj; ++i)
            {
                // every call of one iteration of src/main.cpp:98-105 between two clock reads (~20 ns each)
                const auto c0 = clock::now();
                auto p = paris::backend::make_projection_host(src_det.n_row, src_det.n_col);
                const auto c1 = clock::now();
                std::memcpy(p.buf.get(), frames.data() + frame * (i % n_held), frame * sizeof(float));
                const auto c2 = clock::now();
                p.idx = i;
                auto d_p = paris::load(p);
                if(binning) // the loaded source frame into a buffer of the binned detector, which takes its place
                {
                    auto d_b = paris::backend::make_projection_device(det.n_row, det.n_col);
                    d_b.idx = d_p.idx;
                    d_b.phi = d_p.phi;
                    d_b.meta = d_p.meta;
                    paris::backend::bin_frame(d_p.buf.get(), d_p.buf.pitch(), d_b.buf.get(), d_b.buf.pitch(), src_det.n_row, src_det.n_col, det.n_col);
                    d_p = std::move(d_b);
                }
                if(lag) // on the counts, before paris::weight() corrects them to line integrals
                    paris::backend::lag_correct(d_p.buf.get(), d_p.buf.pitch(), det.n_row, det.n_col, 0u, det.n_col);
                const auto c3 = clock::now();
                if(do_weight) paris::weight(d_p, det);
                const auto c4 = clock::now();
                if(do_filter) paris::filter(d_p, det);
                const auto c5 = clock::now();
                paris::backproject(d_p, v, offset, det, vol_geo, false, enable_roi, roi);
                const auto c6 = clock::now();
                d_p.buf = paris::backend::projection_device_buffer_type{}; // (what the end of the reference's loop body does)
                const auto c7 = clock::now();
                p.buf.reset();
                if(clear_after >= 0 && i == static_cast<std::uint32_t>(clear_after))
                    clear_set();
                const auto c8 = clock::now();
                const clock::time_point c[9] = {c0, c1, c2, c3, c4, c5, c6, c7, c8};
                for(int k = 0; k < 8; ++k)
                    split_s[k] += std::chrono::duration<double>(c[k + 1] - c[k]).count();
            }
            if(lag)
                paris::backend::lag_end();
            fill_s = split_s[1];
            const auto t_tail = std::chrono::steady_clock::now();
            paris::backend::synchronize(); // the timed region ends when the GPU has finished, not when the last call returned
            tail_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_tail).count();
            loop_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
            auto filtered = paris::backend::volume_device_type{}; // --denoise: what is read back in v's place
            if(!voxel_index_path.empty()) // the slab's part of the metal voxels, into the finished slab
                paris::backend::metal_reinsert(v.buf.get(), v.dim_x, v.dim_y, v.dim_z, offset);
            if(denoise) // one slab: the whole volume, filtered in two ranges of slices that both read all of it
            {
                filtered = paris::backend::make_volume_device(v.dim_x, v.dim_y, v.dim_z);
                const auto h = v.dim_z / 2u;
                paris::backend::volume_bilateral(v.buf.get(), v.dim_x, v.dim_y, v.dim_z, 0u, h, denoise_sigma_r, denoise_sigma_s, denoise_radius,
                                                 filtered.buf.get());
                paris::backend::volume_bilateral(v.buf.get(), v.dim_x, v.dim_y, v.dim_z, h, v.dim_z - h, denoise_sigma_r, denoise_sigma_s, denoise_radius,
                                                 filtered.buf.get() + std::size_t{h} * v.dim_x * v.dim_y);
            }
            if(!reproject_path.empty()) // this slab's part of every view, while its volume is alive
            {
                const float delta_s = det.delta_s * det.l_px_row, delta_t = det.delta_t * det.l_px_col; // src/backprojection.cpp:49-50
                for(std::uint32_t i = 0; i < n_proj; ++i)
                {
                    float sin_phi = 0.f, cos_phi = 0.f;
                    paris::backend::detail::runtime_check(paris_hip_stage_angle(&det, i, 0, 0.f, &sin_phi, &cos_phi), "--reproject");
                    auto h_p = paris::backend::make_projection_host(det.n_row, det.n_col);
                    auto d_p = paris::backend::make_projection_device(det.n_row, det.n_col);
                    if(id > 0)
                    {
                        std::memcpy(h_p.buf.get(), reprojected.data() + frame * i, frame * sizeof(float));
                        paris::backend::copy_h2d(h_p, d_p);
                    }
                    paris::backend::forward_project(v, offset, det, vol_geo, d_p, sin_phi, cos_phi, delta_s, delta_t, id > 0);
                    paris::backend::copy_d2h(d_p, h_p);
                    std::memcpy(reprojected.data() + frame * i, h_p.buf.get(), frame * sizeof(float));
                }
            }
            if(out == nullptr) // --no-out: a throughput run, the volume is neither read back nor written
                continue;
            auto h_v = paris::backend::make_volume_host(v.dim_x, v.dim_y, v.dim_z);
            paris::backend::copy_d2h(denoise ? filtered : v, h_v);
            const auto n = std::size_t{v.dim_x} * v.dim_y * v.dim_z;
            std::fseek(out, static_cast<long>(std::size_t{v.dim_x} * v.dim_y * offset * sizeof(float)), SEEK_SET);
            if(std::fwrite(h_v.buf.get(), sizeof(float), n, out) != n)
                throw paris::stage_runtime_error{"short write"};
        }
        if(out != nullptr)
            std::fclose(out);
        if(!reproject_path.empty())
        {
            std::FILE* f = std::fopen(reproject_path.c_str(), "wb");
            if(f == nullptr || std::fwrite(reprojected.data(), sizeof(float), reprojected.size(), f) != reprojected.size())
                throw paris::stage_runtime_error{"cannot write " + reproject_path};
            std::fclose(f);
        }
        if(air)
        {
            const auto c = paris::backend::air_stats();
            std::printf("air: %llu frames, %llu normalised, %llu too few, %llu above the limit, values %.9g .. %.9g\n",
                        static_cast<unsigned long long>(c.frames), static_cast<unsigned long long>(c.normalised), static_cast<unsigned long long>(c.too_few),
                        static_cast<unsigned long long>(c.above_limit), static_cast<double>(c.min_a), static_cast<double>(c.max_a));
        }
        std::printf("ok %u %u %u\n", roi_geo.dim_x, roi_geo.dim_y, roi_geo.dim_z);
        std::printf("projection loops %.3f s: %.1f GVoxel-updates/s through paris::load / weight / filter / backproject (deferral depth %d, %s)\n", loop_s,
                    static_cast<double>(roi_geo.dim_x) * roi_geo.dim_y * roi_geo.dim_z * n_proj / loop_s / 1e9, PARIS_HIP_BACKPROJECT_DEFERRAL,
                    PARIS_HIP_BACKPROJECT_OVERLAP ? (PARIS_HIP_UPLOAD_ON_ITS_OWN_STREAM ? "fused launches on the second stream, uploads on the upload stream"
                                                                                         : "fused launches on the second stream, uploads on the compute stream")
                                                  : "one stream");
        std::printf("of which: host frame fill (memcpy into the pinned buffer) %.3f s, backend calls %.3f s, final wait for the GPU %.3f s\n", fill_s,
                    loop_s - fill_s - tail_s, tail_s);
        {
            const double per = 1e6 / (static_cast<double>(n_proj) * info.num);
            std::printf("per projection [us]: make_projection_host %.2f, frame fill %.2f, load (make_projection_device + copy_h2d) %.2f, weight %.2f, filter %.2f, "
                        "backproject %.2f, free device buffer %.2f, free host buffer %.2f\n", split_s[0] * per, split_s[1] * per, split_s[2] * per,
                        split_s[3] * per, split_s[4] * per, split_s[5] * per, split_s[6] * per, split_s[7] * per);
        }
        if(json)
        {
            const double per = 1e6 / (static_cast<double>(n_proj) * info.num);
            // what the device holds when the loops are over (the last slab's volume has been released by now): the library's parked
            // projection buffers and tables -- bounded, however many projections went through
            std::size_t mem_free = 0, mem_total = 0;
            (void)paris_hip_device_memory(devices[0], &mem_free, &mem_total);
            std::printf("{\"volume\": [%u, %u, %u], \"projections\": %u, \"frame\": [%u, %u], \"slabs\": %d, \"seconds\": %.6f, \"value\": %.3f, "
                        "\"unit\": \"GVoxel-updates/s\", \"host_fill_seconds\": %.6f, \"backend_call_seconds\": %.6f, \"final_wait_seconds\": %.6f, "
                        "\"deferral\": %d, \"streams\": \"%s\", \"filter_deferral\": %d, \"by_reference\": %d, \"device_bytes_in_use_after_the_loops\": %zu, \"us_per_projection\": {\"make_projection_host\": %.3f, "
                        "\"frame_fill\": %.3f, \"load\": %.3f, \"weight\": %.3f, \"filter\": %.3f, \"backproject\": %.3f, \"free_device\": %.3f, "
                        "\"free_host\": %.3f}}\n", roi_geo.dim_x, roi_geo.dim_y, roi_geo.dim_z, n_proj, det.n_row, det.n_col, info.num, loop_s,
                        static_cast<double>(roi_geo.dim_x) * roi_geo.dim_y * roi_geo.dim_z * n_proj / loop_s / 1e9, fill_s, loop_s - fill_s - tail_s, tail_s,
                        PARIS_HIP_BACKPROJECT_DEFERRAL, PARIS_HIP_BACKPROJECT_OVERLAP ? (PARIS_HIP_UPLOAD_ON_ITS_OWN_STREAM ? "compute + second (fused launches) + upload" : "compute (copies) + second (filter, fused launches)") : "one",
                        PARIS_HIP_FILTER_DEFERRAL, PARIS_HIP_BACKPROJECT_REFERENCES, mem_total - mem_free, split_s[0] * per, split_s[1] * per, split_s[2] * per, split_s[3] * per, split_s[4] * per,
                        split_s[5] * per, split_s[6] * per, split_s[7] * per);
        }
        return 0;
    }
    catch(const paris::stage_construction_error& e)
    {
        std::fprintf(stderr, "pipeline construction failed: %s\n", e.what());
        return 1;
    }
    catch(const paris::stage_runtime_error& e)
    {
        std::fprintf(stderr, "pipeline execution failed: %s\n", e.what());
        return 1;
    }
}

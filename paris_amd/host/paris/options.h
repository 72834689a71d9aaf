// The driver's options: what paris.hip can be told (program_options), how each option's value is read as typed (parse_*, behind the
// table find_option_parser looks flags up in) and how run() checks a setting before any device work (check_*). Every parse_* is
// colon_fields, a test of the field count, then the two field readers -- read_number and read_unsigned --, so that every option
// reads a number or an unsigned integer by the same rule; demo/paris_hip_options prints what a value sets, and
// tests/test_options_host.py holds it to expectations written down by hand.
#ifndef PARIS_AMD_HOST_OPTIONS_H_
#define PARIS_AMD_HOST_OPTIONS_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "source.h"
#include "types.h"

namespace paris
{
    // --voxel-type / --voxel-range as given (program_options, below); what a drain thread needs to know about the output
    struct voxel_output
    {
        int type = 0;             // 0: float voxels into the DDBVF; PARIS_HIP_VOXEL_U8 / _U16
        bool range_given = false; // --voxel-range was given
        bool automatic = false;   // ... as auto
        float lo = 0.f, hi = 0.f;
        double p_lo = 0.1, p_hi = 99.9;
    };

    // src/program_options.h:34-50 (the parts the hot path needs)
    struct program_options
    {
        detector_geometry det_geo{};
        bool enable_io = false;
        std::string input_path, output_path, prefix = "vol";
        bool enable_roi = false;
        region_of_interest roi{};
        bool enable_angles = false;
        std::string angle_path;
        std::uint16_t quality = 1;
        int slabs = 0;     // 0: memory driven (reference behaviour); > 0: fixed slab count
        int devices = 0;   // 0: all
        int slots = 4;     // pinned upload buffers per device
        bool f16 = false;  // store filtered projections as IEEE half before backprojection (BASELINE config 5)
        int batch = 32;    // projections per fused backprojection launch, up to 64 (1: one launch per projection, as the reference)
        // pinned staging per buffer for the volume's way to the file: small, because pinning costs more than it saves (two
        // 256 MiB buffers added 0.4 s to a 1.3 s reconstruction; 16 MiB chunks still run the copy at full rate)
        std::size_t drain_chunk_bytes = std::size_t{16} << 20;
        int window = PARIS_HIP_WINDOW_RAMP; // filter window (extension: PARIS_HIP_WINDOW_SHEPP_LOGAN; the reference has the ramp only)
        bool row_band = true; // f4: per slab, upload / weight / filter only the detector rows the slab can read
        // several devices: 1 = the device threads of a pass share one read-once frame source (source.h: shared_frames), 0 = each reads
        // the files through a stream of its own (only its slab's detector rows when row_band is on), -1 = decided by how many
        // detector rows the slabs of a pass need between them (run())
        int share_frames = -1;
        bool read_ahead = true;  // frames are read and converted by a feed thread per device, ahead of the device thread
        bool two_volumes = true; // a device with several slabs to do keeps two volume buffers when memory allows (drain thread, below)
        // memory-driven split that gives every device one slab of at least 1 GiB: cut each into this many (0: leave it), so that all
        // but the last of a device's slabs go to the file while the next one is reconstructed
        int pipeline_slabs = 4;
        // Parker redundancy weighting of a short scan (extension): [start, start + range] is derived by run() from the first and last
        // angle of the frames the run uses, before any device work (detail::derive_short_scan)
        bool short_scan = false;
        paris_short_scan scan{};
        // redundancy weighting of an offset-detector (half-fan) full circle (extension): run() checks the detector's overlap and that
        // the frames cover the circle, before any device work (detail::check_offset_detector)
        bool offset_detector = false;
        // dark / flat correction of intensity frames to line integrals (extension): --flat / --dark name HIS files whose frames are
        // averaged into one reference frame each by run(), before any device work (detail::load_flat_field); every device ctx gets
        // them and uploads frames through the corrected upload (detail::frame_chain::upload)
        std::string flat_path, dark_path;
        float t_min = 1e-5f;
        std::shared_ptr<const his::mean> flat, dark; // filled by run(); dark may stay empty (a zero dark)
        // repair of defective detector pixels (extension): --defects names a file of n_col x n_row raw bytes
        // (nonzero = defective), read by run() before any device work (detail::load_defects); --defects-from-flat ORs in the pixels
        // the flat-field setting finds dead (paris_hip_flat_field_dead_pixels; needs --flat). Every device ctx gets the map, and each
        // frame is repaired after the dark / flat correction and before the weights
        std::string defects_path;
        bool defects_from_flat = false;
        std::shared_ptr<const std::vector<std::uint8_t>> defect_mask; // filled by run() from --defects
        std::size_t defect_bytes = 0; // filled by run(): what the plan of --defects occupies on a device
        // removal of per-frame outlier pixels (extension): --zingers ABS[:REL] and --zinger-polarity
        // bright|dark|both (default: dark with --flat, where a hit's high count is a deep negative line integral, else bright), checked
        // by run() before any device work (detail::check_zingers). Every device ctx gets the setting, and each frame is filtered after
        // the defect repair and before the weights
        bool zingers = false;
        float zinger_abs = 0.f, zinger_rel = 0.f;
        int zinger_polarity = 2;      // +1 bright, -1 dark, 0 both; 2: the default, resolved by run()
        std::size_t zinger_bytes = 0; // filled by run(): what the setting occupies on a device
        // normalisation of every frame to an air region (extension): --air-region X0:Y0:W:H[:LIMIT], a rectangle
        // of the frame the reconstruction sees (the binned frame with --bin) that sees only air in every view, checked by run()
        // before any device work (detail::check_air_region). Every device ctx gets the setting, with the defect map's mask if there
        // is one, and each frame has the rectangle's mean line integral subtracted directly after the correction
        bool air = false;
        paris_hip_air_region air_region{};
        std::size_t air_bytes = 0; // filled by run(): what the setting occupies on a device
        // removal of ring artefacts (extension): --rings H[:FLOOR[:LIMIT]], checked by run() before any device
        // work (detail::check_rings). run() then reads the scan once on the first device (detail::ring_prepass): every frame goes
        // through the chain the reconstruction uses -- correction, repair, zinger filter -- into the profile, and the rule's correction
        // frame is kept here. Every device ctx gets it, and each frame is corrected after the zinger filter and before the weights
        bool rings = false;
        std::uint32_t ring_half_width = 0;
        float ring_floor = 0.f, ring_limit = 0.f;
        std::size_t ring_bytes = 0;                             // filled by run(): what the correction frame occupies on a device
        std::shared_ptr<const std::vector<float>> ring_c;       // filled by run(): the correction frame
        // the rotation axis from the scan itself (extension): --find-axis LO:HI[:STEP] [--axis-rows R]
        // [--axis-only], checked by run() before any device work (detail::check_axis). run() then reads the scan once on the first
        // device (detail::prepass, the ring filter's pre-pass: with --rings each group of frames feeds both), scores the candidates
        // and replaces det_geo.delta_s by the estimate before anything is derived from it
        bool find_axis = false, axis_only = false;
        float axis_lo = 0.f, axis_hi = 0.f, axis_step = 0.25f;
        std::uint32_t axis_rows = 2;
        bool axis_rows_given = false;
        std::uint32_t axis_count = 0, axis_frames = 0;          // filled by run(): the candidates, and the frames of the circle
        // beam-hardening correction (extension): --beam-hardening C1:C2[:C3[:C4]] gives the polynomial of the
        // line integral, --fit-beam-hardening N[:SLICES[:MARGIN]] has run() fit it from the scan itself (detail::bh_prepass, after the
        // ring pre-pass and the axis search): both checked by run() before any device work (detail::check_beam_hardening). Every
        // device ctx gets the setting, and each frame is corrected after the ring correction and before every weight
        bool beam_hardening = false, fit_beam_hardening = false;
        paris_hip_beam_hardening bh{};                          // as given, or filled by run() with the fitted coefficients
        std::uint32_t bh_slices = 32, bh_margin = 2;            // the fit's slab -- the central slices of the volume -- and its margin
        // single-distance phase retrieval (extension): --phase DELTA_BETA:ENERGY_KEV[:MARGIN] gives the material
        // and the energy, --phase-alpha MM2[:MARGIN] the filter's alpha at the detector plane itself; --phase-floor T the floor of the
        // retrieved transmission (default: the flat field's t_min, else 1e-6). Checked by run() before any device work, for the binned
        // detector with --bin (detail::check_phase). Every device ctx gets the setting, and each frame is filtered -- as a whole: the run
        // is planned without the row band -- after the ring correction and before the beam-hardening polynomial
        bool phase = false, phase_material = false, phase_floor_given = false;
        double phase_delta_beta = 0.0, phase_energy = 0.0;
        std::uint32_t phase_margin = 0;                         // 0: not given; run() takes paris_hip_phase_default_margin
        paris_hip_phase_retrieval phase_setting{};              // alpha as given; the rest filled by run()
        std::uint32_t phase_nx = 0, phase_ny = 0;               // filled by run(): the padded size
        std::size_t phase_scratch = 0, phase_bytes = 0;         // filled by run(): the scratch, and what the setting occupies on a device
        // scatter correction (extension): --scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2] gives the source and
        // the kernel (without the last two fields one Gaussian: W2 = 0, SIGMA2 = SIGMA1), --scatter-iterations N, --scatter-limit F and
        // --scatter-margin M the rest (defaults 4, 0.8 and paris_hip_scatter_default_margin). Checked by run() before any device work,
        // for the binned detector with --bin (detail::check_scatter). Every device ctx gets the setting, and each frame is corrected -- as
        // a whole: the run is planned without the row band -- after the ring correction and before the phase retrieval
        bool scatter = false, scatter_detail_given = false;     // the latter: one of the three options beside --scatter was given
        paris_hip_scatter_correction scatter_setting{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.8f, 4u, 0u}; // margin 0: not given; run() takes the default
        std::uint32_t scatter_nx = 0, scatter_ny = 0;           // filled by run(): the padded size
        std::size_t scatter_scratch = 0, scatter_bytes = 0;     // filled by run(): the scratch, and what the setting occupies on a device
        // suppression of photon-starvation streaks (extension): --starvation P0[:GAIN[:RADIUS]] gives the line
        // integral above which a pixel is smoothed, the scale of the width law (default 1) and the stencil's radius (default 3). Checked by
        // run() before any device work, for the binned detector with --bin (detail::check_starvation). Every device ctx gets the setting,
        // and each frame is filtered -- as a whole: the run is planned without the row band -- after the ring correction and before the
        // scatter correction
        bool starvation = false;
        paris_hip_starvation_filter starvation_setting{0.f, 1.f, 3u};
        std::size_t starvation_bytes = 0;                       // filled by run(): what the setting occupies on a device
        // correction of the detector's in-plane rotation (extension): --detector-roll DEG gives the angle,
        // --find-roll LO:HI[:STEP] [--roll-only] has run() find it from the scan mean of the ring profile pre-pass (detail::prepass,
        // after the axis search, whose delta_s it uses): both checked by run() before any device work (detail::check_roll). Every
        // device ctx gets the setting, and each frame is resampled into a second buffer of its slot after the beam-hardening
        // correction and before every weight; everything after reads that buffer
        bool roll = false, find_roll = false, roll_only = false;
        float roll_deg = 0.f;                                   // as given, or filled by run() with the estimate
        float roll_lo = 0.f, roll_hi = 0.f, roll_step = 0.25f;
        std::uint32_t roll_count = 0;                           // filled by run(): the candidates
        // detector binning (extension): --bin BX[:BY], each 1, 2, 4 or 8; 1 x 1 is no binning. run() checks the
        // setting before any device work and replaces det_geo by the binned geometry (detail::apply_binning), so that everything
        // derived from it follows; the dark and flat means and the defect mask are binned on the host, the frames on the device, each
        // between its raw upload into a full-width slot and the correction
        std::uint32_t bin_x = 1, bin_y = 1;
        std::uint32_t src_row = 0, src_col = 0;                         // filled by run() with binning: the source detector (0: no binning)
        std::shared_ptr<const std::vector<std::uint8_t>> bin_mask;      // filled by run(): the bad source pixels left out of their bins (may be empty)
        bool binning() const { return src_row != 0; }
        // correction of the detector's lag (extension): --lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]] gives the weights and
        // decay rates per frame of the panel's impulse response, --lag-start rest|steady how a pass over the scan starts (steady: the
        // beam was on before the first frame, the default), checked by run() before any device work (detail::check_lag): it needs
        // --flat, because the frames must be counts, and every frame of the scan (no --quality above 1). Every device ctx gets the
        // setting; each pass over the scan opens a sequence for the rows it uploads, corrects every frame between its raw upload (and
        // binning) and the dark / flat correction, which then runs as a pass of its own, and closes the sequence after the last frame
        bool lag = false, lag_start_given = false;
        paris_hip_lag_model lag_model{0u, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, PARIS_HIP_LAG_START_STEADY};
        // metal artefact reduction by linear interpolation (extension): --metal THR[:GROW[:MIN_PATH]] -- THR in
        // the volume's own units, GROW pixels the trace is widened by (default 1), MIN_PATH [mm] of metal a ray must cross (default:
        // half the smallest voxel edge) -- checked by run() before any device work (detail::check_metal). run() then reconstructs the
        // scan once on the first device (detail::metal_prepass, after every other pre-pass, with their results in force), collects
        // the voxels above THR, forward-projects their mask and packs the traces. Every device ctx gets the traces and the list; each
        // frame is inpainted after the roll and before the redundancy weights, and each slab gets its metal voxels back at its end
        bool metal = false;
        float metal_threshold = 0.f, metal_min_path = -1.f;     // min_path < 0: not given; run() resolves it from the voxel size
        std::uint32_t metal_grow = 1;
        std::uint32_t metal_views = 0;                          // filled by run(): the views the traces cover
        std::shared_ptr<const std::vector<std::uint64_t>> metal_bits, metal_index; // filled by run(): the packed traces; the list's indices
        std::shared_ptr<const std::vector<float>> metal_value;  // filled by run(): the list's values
        std::size_t metal_bytes = 0;                            // filled by run(): what both settings occupy on a device
        // edge-preserving denoising of the finished volume (extension): --denoise SIGMA_R[:SIGMA_S[:RADIUS]] --
        // SIGMA_R in the volume's own units, SIGMA_S in voxels (default 1), RADIUS 1 .. 3 (default min(3, ceil(2 SIGMA_S))) -- checked by
        // run() before any device work (detail::check_denoise). Every slab is then reconstructed with up to RADIUS halo slices on each
        // side, clamped to the output grid, and the drain thread filters each chunk of whole slices into a scratch before it copies
        // (or quantises) it down: the file does not depend on slabs, devices or the chunk size
        bool denoise = false, denoise_radius_given = false;
        struct paris_hip_volume_bilateral denoise_setting{0.f, 1.f, 0u}; // (`struct`: the entry point has the type's name)
        std::size_t denoise_bytes = 0; // filled by run(): the halo slices of a slab, the drain ctx's scratch and its tables
        // row extension for laterally truncated projections (extension): --extend-rows W[:M], the taper length
        // and the number of edge pixels averaged (default 4), checked by run() before any device work (detail::check_extend_rows).
        // Every device ctx gets the setting; the row filter then adds the rank-2 update at its store
        bool extend_rows = false;
        std::uint32_t extend_taper = 0, extend_edge = 4;
        std::size_t extend_bytes = 0; // filled by run(): the response vector a device keeps while set
        // voxels written as 8- or 16-bit integers over a grey window (extension): --voxel-type u8|u16 with
        // --voxel-range LO:HI or auto[:P_LO:P_HI], checked by run() before any device work (detail::check_voxels). The drain threads
        // then quantise each chunk on the device and copy 1 or 2 bytes per voxel down; the file is <name>.raw with <name>.mhd beside
        // it. auto: the window between two percentiles of the finished volume's histogram -- one slab on one device only.
        // Without --voxel-type (0) the float DDBVF is written as ever.
        voxel_output voxels;
    };

    namespace detail
    {
        // the fields of a colon-separated option value; an empty field stays in as an empty string
        inline auto colon_fields(const std::string& v) -> std::vector<std::string>
        {
            auto out = std::vector<std::string>{};
            std::size_t at = 0;
            for(;;)
            {
                const auto next = v.find(':', at);
                out.push_back(v.substr(at, next == std::string::npos ? next : next - at));
                if(next == std::string::npos)
                    return out;
                at = next + 1u;
            }
        }

        // what a parser throws for a value it cannot read: the option's usage, then the value as typed
        inline auto cannot_read(const std::string& usage, const std::string& v) -> stage_construction_error
        {
            return stage_construction_error{usage + ": cannot read '" + v + "'"};
        }

        // One number from a field, float or double: the field must not be empty and strtof / strtod must consume all of it, or `bad` is
        // thrown. Leading blanks, inf, nan and hex floats pass; text outside the type's range becomes inf, 0 or a subnormal, which is
        // for the option's check_* to judge.
        template<class T>
        inline auto read_number(const std::string& field, const stage_construction_error& bad) -> T
        {
            static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value, "a float or a double");
            char* end = nullptr;
            const T x = std::is_same<T, float>::value ? static_cast<T>(std::strtof(field.c_str(), &end)) : static_cast<T>(std::strtod(field.c_str(), &end));
            if(field.empty() || *end != '\0')
                throw bad;
            return x;
        }

        // one unsigned integer from a field: 1 to 9 decimal digits and nothing else, or `bad` is thrown
        inline auto read_unsigned(const std::string& field, const stage_construction_error& bad) -> std::uint32_t
        {
            if(field.empty() || field.size() > 9u || field.find_first_not_of("0123456789") != std::string::npos)
                throw bad;
            return static_cast<std::uint32_t>(std::stoul(field));
        }

        // --bin BX[:BY] as typed; BY defaults to BX
        inline auto parse_bin(const std::string& v, program_options& po) -> void
        {
            const auto field = colon_fields(v);
            const auto factor = [&](const std::string& t) -> std::uint32_t {
                if(field.size() > 2u || (t != "1" && t != "2" && t != "4" && t != "8"))
                    throw stage_construction_error{"--bin BX[:BY]: each factor is 1, 2, 4 or 8 (got '" + v + "')"};
                return static_cast<std::uint32_t>(t[0] - '0');
            };
            po.bin_x = factor(field[0]);
            po.bin_y = field.size() > 1u ? factor(field[1]) : po.bin_x;
        }

        // --zingers ABS[:REL] as typed; refuses anything that is not one or two numbers
        inline auto parse_zingers(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--zingers ABS[:REL]", v);
            const auto field = colon_fields(v);
            if(field.size() > 2u)
                throw bad;
            po.zinger_abs = read_number<float>(field[0], bad);
            po.zinger_rel = field.size() > 1u ? read_number<float>(field[1], bad) : 0.f;
            po.zingers = true;
        }

        inline auto parse_zinger_polarity(const std::string& v, program_options& po) -> void
        {
            if(v == "bright") po.zinger_polarity = 1;
            else if(v == "dark") po.zinger_polarity = -1;
            else if(v == "both") po.zinger_polarity = 0;
            else throw stage_construction_error{"--zinger-polarity bright|dark|both: unknown polarity " + v};
        }

        // --zingers / --zinger-polarity: the default polarity is resolved and the setting checked here, before any device work
        inline auto check_zingers(program_options& po) -> void
        {
            if(!po.zingers)
            {
                if(po.zinger_polarity != 2)
                    throw stage_construction_error{"--zinger-polarity needs --zingers"};
                return;
            }
            if(po.zinger_polarity == 2)
                po.zinger_polarity = po.flat_path.empty() ? 1 : -1;
            const auto setting = paris_hip_zinger_filter{po.zinger_abs, po.zinger_rel, po.zinger_polarity, 0u};
            const int rc = paris_hip_zinger_filter_check(&setting, po.det_geo.n_row, po.det_geo.n_col, nullptr, &po.zinger_bytes);
            if(rc == PARIS_HIP_ERROR_UNSUPPORTED)
                throw stage_construction_error{"--zingers: the detector has more than 2^32 - 1 pixels"};
            if(rc != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--zingers ABS[:REL]: the thresholds must be finite, not negative and not both zero (got "
                                               + std::to_string(po.zinger_abs) + ":" + std::to_string(po.zinger_rel) + ")"};
        }

        // --voxel-type u8|u16 as typed
        inline auto parse_voxel_type(const std::string& v, program_options& po) -> void
        {
            if(v == "u8") po.voxels.type = PARIS_HIP_VOXEL_U8;
            else if(v == "u16") po.voxels.type = PARIS_HIP_VOXEL_U16;
            else throw stage_construction_error{"--voxel-type u8|u16: unknown type " + v};
        }

        // --voxel-range LO:HI or auto[:P_LO:P_HI] as typed; refuses anything else
        inline auto parse_voxel_range(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--voxel-range LO:HI | auto[:P_LO:P_HI]", v);
            const auto field = colon_fields(v);
            const bool automatic = field[0] == "auto";
            if(automatic ? field.size() != 1u && field.size() != 3u : field.size() != 2u)
                throw bad;
            if(!automatic)
            {
                po.voxels.lo = static_cast<float>(read_number<double>(field[0], bad));
                po.voxels.hi = static_cast<float>(read_number<double>(field[1], bad));
            }
            else if(field.size() == 3u)
            {
                po.voxels.p_lo = read_number<double>(field[1], bad);
                po.voxels.p_hi = read_number<double>(field[2], bad);
            }
            po.voxels.automatic = automatic;
            po.voxels.range_given = true;
        }

        // --voxel-type / --voxel-range: both or neither, a window the library accepts, and auto only where one drain thread sees the
        // whole volume -- here, before any device work and before the output directory is made
        inline auto check_voxels(const program_options& po) -> void
        {
            if(po.voxels.type == 0 && !po.voxels.range_given)
                return;
            if(po.voxels.type == 0)
                throw stage_construction_error{"--voxel-range needs --voxel-type u8|u16"};
            if(!po.voxels.range_given)
                throw stage_construction_error{"--voxel-type needs --voxel-range LO:HI | auto[:P_LO:P_HI]"};
            if(po.voxels.automatic)
            {
                if(!(po.voxels.p_lo >= 0.0) || !(po.voxels.p_lo < po.voxels.p_hi) || !(po.voxels.p_hi <= 100.0))
                    throw stage_construction_error{"--voxel-range auto:P_LO:P_HI: the percentiles must satisfy 0 <= P_LO < P_HI <= 100"};
                if(po.slabs != 1)
                    throw stage_construction_error{"--voxel-range auto needs the whole volume in one slab on one device: give --slabs 1 (and --devices 1)"};
                return;
            }
            const auto window = paris_hip_volume_window{po.voxels.lo, po.voxels.hi, po.voxels.type};
            if(paris_hip_volume_window_check(&window) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--voxel-range LO:HI: LO and HI must be finite, with HI > LO by at least 2^-100 (got " + std::to_string(po.voxels.lo)
                                               + ":" + std::to_string(po.voxels.hi) + ")"};
        }

        // --air-region X0:Y0:W:H[:LIMIT] as typed; refuses anything but four unsigned integers and an optional number
        inline auto parse_air_region(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--air-region X0:Y0:W:H[:LIMIT]", v);
            const auto field = colon_fields(v);
            if(field.size() != 4u && field.size() != 5u)
                throw bad;
            std::uint32_t rect[4] = {0, 0, 0, 0};
            for(int k = 0; k < 4; ++k)
                rect[k] = read_unsigned(field[k], bad);
            const float limit = field.size() == 5u ? read_number<float>(field[4], bad) : 0.f;
            po.air_region = paris_hip_air_region{rect[0], rect[1], rect[2], rect[3], 0u, limit};
            po.air = true;
        }

        // --air-region: the rectangle is checked against the detector the reconstruction sees (binned with --bin) here, before any
        // device work
        inline auto check_air_region(program_options& po) -> void
        {
            if(!po.air)
                return;
            if(paris_hip_air_region_check(&po.air_region, po.det_geo.n_row, po.det_geo.n_col, nullptr, &po.air_bytes) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--air-region X0:Y0:W:H[:LIMIT]: W and H at least 1, the rectangle inside the " + std::to_string(po.det_geo.n_row)
                                               + " x " + std::to_string(po.det_geo.n_col) + " frame, at most 2^20 pixels, LIMIT finite and not negative (got "
                                               + std::to_string(po.air_region.x0) + ":" + std::to_string(po.air_region.y0) + ":"
                                               + std::to_string(po.air_region.width) + ":" + std::to_string(po.air_region.height) + ":"
                                               + std::to_string(po.air_region.limit_abs) + ")"};
        }

        // --extend-rows W[:M] as typed; refuses anything that is not one or two unsigned integers
        inline auto parse_extend_rows(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--extend-rows W[:M]", v);
            const auto field = colon_fields(v);
            if(field.size() > 2u)
                throw bad;
            po.extend_taper = read_unsigned(field[0], bad);
            po.extend_edge = field.size() > 1u ? read_unsigned(field[1], bad) : 4u;
            po.extend_rows = true;
        }

        // --extend-rows: the setting is checked for this detector here, before any device work
        inline auto check_extend_rows(program_options& po) -> void
        {
            if(!po.extend_rows)
                return;
            const auto setting = paris_hip_row_extension{po.extend_edge, po.extend_taper};
            if(paris_hip_row_extension_check(&setting, po.det_geo.n_row) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--extend-rows W[:M]: W must lie in 1 .. 16384 and M must be 1, 2, 4 or 8 and at most n_row (got "
                                               + std::to_string(po.extend_taper) + ":" + std::to_string(po.extend_edge) + ")"};
            po.extend_bytes = std::size_t{po.det_geo.n_row} * sizeof(float);
        }

        // --rings H[:FLOOR[:LIMIT]] as typed; refuses anything that is not an unsigned integer and up to two numbers
        inline auto parse_rings(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--rings H[:FLOOR[:LIMIT]]", v);
            const auto field = colon_fields(v);
            if(field.size() > 3u)
                throw bad;
            po.ring_half_width = read_unsigned(field[0], bad);
            po.ring_floor = field.size() > 1u ? read_number<float>(field[1], bad) : 0.f;
            po.ring_limit = field.size() > 2u ? read_number<float>(field[2], bad) : 0.f;
            po.rings = true;
        }

        // --rings: the setting is checked for this detector here, before any device work
        inline auto check_rings(program_options& po) -> void
        {
            if(!po.rings)
                return;
            const auto setting = paris_hip_ring_filter{po.ring_half_width, po.ring_floor, po.ring_limit};
            const int rc = paris_hip_ring_filter_check(&setting, po.det_geo.n_row, po.det_geo.n_col, nullptr, &po.ring_bytes);
            if(rc == PARIS_HIP_ERROR_UNSUPPORTED)
                throw stage_construction_error{"--rings: the detector has more than 2^32 - 1 pixels"};
            if(rc != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--rings H[:FLOOR[:LIMIT]]: H must lie in 1 .. 32, FLOOR must be finite and not negative, LIMIT 0 (none) or "
                                               "finite and above FLOOR (got " + std::to_string(po.ring_half_width) + ":" + std::to_string(po.ring_floor)
                                               + ":" + std::to_string(po.ring_limit) + ")"};
        }

        // --starvation P0[:GAIN[:RADIUS]] as typed; refuses anything but one or two numbers and an unsigned integer
        inline auto parse_starvation(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--starvation P0[:GAIN[:RADIUS]]", v);
            const auto field = colon_fields(v);
            if(field.size() > 3u)
                throw bad;
            auto& s = po.starvation_setting;
            s.p0 = read_number<float>(field[0], bad);
            s.gain = field.size() > 1u ? read_number<float>(field[1], bad) : 1.f;
            s.radius = field.size() > 2u ? read_unsigned(field[2], bad) : 3u;
            po.starvation = true;
        }

        // --starvation: checked here for the detector the reconstruction sees (the binned one with --bin), before any device work. The
        // pass has no row band: the run is planned as --no-row-band plans it.
        inline auto check_starvation(program_options& po) -> void
        {
            if(!po.starvation)
                return;
            const auto& s = po.starvation_setting;
            const int rc = paris_hip_starvation_filter_check(&s, po.det_geo.n_row, po.det_geo.n_col, &po.starvation_bytes);
            if(rc == PARIS_HIP_ERROR_UNSUPPORTED)
                throw stage_construction_error{"--starvation: the detector has more than 2^32 - 1 pixels"};
            if(rc != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--starvation P0[:GAIN[:RADIUS]]: P0 must be finite, GAIN finite and greater than 0 and RADIUS must lie in 1 .. "
                                               + std::to_string(PARIS_HIP_STARVATION_RADIUS_MAX) + " (got " + std::to_string(s.p0) + ":"
                                               + std::to_string(s.gain) + ":" + std::to_string(s.radius) + ")"};
            if(po.axis_only || po.roll_only)
                throw stage_construction_error{"--starvation cannot be combined with --axis-only or --roll-only: nothing would be reconstructed"};
            po.row_band = false;
        }

        // --scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2] as typed; refuses anything but four or six numbers
        inline auto parse_scatter(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2]", v);
            const auto field = colon_fields(v);
            if(field.size() != 4u && field.size() != 6u)
                throw bad;
            float value[6] = {};
            for(std::size_t k = 0; k < field.size(); ++k)
                value[k] = read_number<float>(field[k], bad);
            auto& s = po.scatter_setting;
            s.amplitude = value[0], s.alpha = value[1], s.beta = value[2], s.sigma1_mm = value[3];
            s.sigma2_mm = field.size() == 6u ? value[4] : value[3];
            s.weight2 = value[5];
            po.scatter = true;
        }

        inline auto parse_scatter_iterations(const std::string& v, program_options& po) -> void
        {
            po.scatter_setting.iterations = read_unsigned(v, cannot_read("--scatter-iterations N", v));
            po.scatter_detail_given = true;
        }

        inline auto parse_scatter_limit(const std::string& v, program_options& po) -> void
        {
            po.scatter_setting.limit = read_number<float>(v, cannot_read("--scatter-limit F", v));
            po.scatter_detail_given = true;
        }

        inline auto parse_scatter_margin(const std::string& v, program_options& po) -> void
        {
            po.scatter_setting.margin = read_unsigned(v, cannot_read("--scatter-margin M", v));
            if(po.scatter_setting.margin == 0u)
                throw stage_construction_error{"--scatter-margin M: M must lie in 1 .. " + std::to_string(PARIS_HIP_PHASE_MARGIN_MAX)};
            po.scatter_detail_given = true;
        }

        // --scatter: resolved and checked here for the detector the reconstruction sees (the binned one with --bin), before any device
        // work. The pass has no row band: the run is planned as --no-row-band plans it.
        inline auto check_scatter(program_options& po) -> void
        {
            if(po.scatter_detail_given && !po.scatter)
                throw stage_construction_error{"--scatter-iterations, --scatter-limit and --scatter-margin need --scatter"};
            if(!po.scatter)
                return;
            auto& s = po.scatter_setting;
            if(s.iterations < 1u || s.iterations > PARIS_HIP_SCATTER_ITERATIONS_MAX)
                throw stage_construction_error{"--scatter-iterations N: N must lie in 1 .. " + std::to_string(PARIS_HIP_SCATTER_ITERATIONS_MAX)};
            if(!(s.limit > 0.f && s.limit < 1.f))
                throw stage_construction_error{"--scatter-limit F: F must lie in (0, 1)"};
            if(s.margin == 0u)
                s.margin = paris_hip_scatter_default_margin(s.sigma1_mm, s.sigma2_mm, po.det_geo.l_px_row, po.det_geo.l_px_col);
            const int rc = paris_hip_scatter_correction_check(&s, po.det_geo.n_row, po.det_geo.n_col, po.det_geo.l_px_row, po.det_geo.l_px_col,
                                                              &po.scatter_nx, &po.scatter_ny, &po.scatter_scratch);
            if(rc == PARIS_HIP_ERROR_UNSUPPORTED)
                throw stage_construction_error{"--scatter: the padded size " + std::to_string(po.scatter_nx) + " x " + std::to_string(po.scatter_ny) + " of a "
                                               + std::to_string(po.det_geo.n_row) + " x " + std::to_string(po.det_geo.n_col) + " frame with a margin of "
                                               + std::to_string(s.margin) + " exceeds " + std::to_string(PARIS_HIP_PHASE_SIZE_MAX)};
            if(rc != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2]: A and the widths must be finite and greater than 0, ALPHA "
                                               "must lie in [-2, 2], BETA in [0, 4], W2 must be finite and not negative, the margin must lie in 1 .. "
                                               + std::to_string(PARIS_HIP_PHASE_MARGIN_MAX) + " and the detector's pixel pitches must be positive (got a margin of "
                                               + std::to_string(s.margin) + ")"};
            po.scatter_bytes = po.scatter_scratch + 12u * (std::size_t{po.scatter_nx} + po.scatter_ny); // twiddles and tables in front of the scratch
            po.row_band = false;
        }

        // --phase DELTA_BETA:ENERGY_KEV[:MARGIN] (material = true) or --phase-alpha MM2[:MARGIN] as typed; refuses anything but the numbers
        // and an unsigned margin
        inline auto parse_phase(const std::string& v, program_options& po, bool material) -> void
        {
            const auto usage = std::string{material ? "--phase DELTA_BETA:ENERGY_KEV[:MARGIN]" : "--phase-alpha MM2[:MARGIN]"};
            const auto bad = cannot_read(usage, v);
            const auto field = colon_fields(v);
            const auto numbers = material ? std::size_t{2} : std::size_t{1};
            if(field.size() < numbers || field.size() > numbers + 1u)
                throw bad;
            double value[2] = {0.0, 0.0};
            for(std::size_t k = 0; k < numbers; ++k)
                value[k] = read_number<double>(field[k], bad);
            po.phase_margin = 0u;
            if(field.size() > numbers)
            {
                po.phase_margin = read_unsigned(field[numbers], bad);
                if(po.phase_margin == 0u)
                    throw stage_construction_error{usage + ": MARGIN must lie in 1 .. " + std::to_string(PARIS_HIP_PHASE_MARGIN_MAX)};
            }
            if(po.phase)
                throw stage_construction_error{"--phase and --phase-alpha cannot be combined: give the material or the filter's alpha"};
            po.phase = true;
            po.phase_material = material;
            po.phase_delta_beta = value[0];
            po.phase_energy = value[1];
            po.phase_setting.alpha_mm2 = material ? 0.f : static_cast<float>(value[0]);
        }

        inline auto parse_phase_floor(const std::string& v, program_options& po) -> void
        {
            po.phase_setting.t_min = read_number<float>(v, cannot_read("--phase-floor T", v));
            po.phase_floor_given = true;
        }

        // --phase / --phase-alpha: resolved and checked here for the detector the reconstruction sees (the binned one with --bin),
        // before any device work. A 2-D filter has no row band: the run is planned as --no-row-band plans it.
        inline auto check_phase(program_options& po) -> void
        {
            if(po.phase_floor_given && !po.phase)
                throw stage_construction_error{"--phase-floor needs --phase or --phase-alpha"};
            if(!po.phase)
                return;
            auto& s = po.phase_setting;
            if(po.phase_material && paris_hip_phase_alpha(&po.det_geo, po.phase_delta_beta, po.phase_energy, &s.alpha_mm2) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--phase DELTA_BETA:ENERGY_KEV[:MARGIN]: both must be finite and greater than 0, and give a finite alpha"};
            if(!(std::isfinite(s.alpha_mm2) && s.alpha_mm2 > 0.f))
                throw stage_construction_error{"--phase-alpha MM2[:MARGIN]: MM2 must be finite and greater than 0"};
            if(!po.phase_floor_given)
                s.t_min = po.flat_path.empty() ? 1e-6f : po.t_min;
            if(!(s.t_min > 0.f && s.t_min <= 1.f))
                throw stage_construction_error{"--phase-floor T: T must lie in (0, 1]"};
            s.margin = po.phase_margin != 0u ? po.phase_margin : paris_hip_phase_default_margin(s.alpha_mm2, po.det_geo.l_px_row, po.det_geo.l_px_col);
            const int rc = paris_hip_phase_retrieval_check(&s, po.det_geo.n_row, po.det_geo.n_col, po.det_geo.l_px_row, po.det_geo.l_px_col, &po.phase_nx,
                                                           &po.phase_ny, &po.phase_scratch);
            if(rc == PARIS_HIP_ERROR_UNSUPPORTED)
                throw stage_construction_error{"--phase: the padded size " + std::to_string(po.phase_nx) + " x " + std::to_string(po.phase_ny) + " of a "
                                               + std::to_string(po.det_geo.n_row) + " x " + std::to_string(po.det_geo.n_col) + " frame with a margin of "
                                               + std::to_string(s.margin) + " exceeds " + std::to_string(PARIS_HIP_PHASE_SIZE_MAX)};
            if(rc != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--phase: MARGIN must lie in 1 .. " + std::to_string(PARIS_HIP_PHASE_MARGIN_MAX) + " and the detector's pixel pitches must be positive (got a margin of "
                                               + std::to_string(s.margin) + ")"};
            po.phase_bytes = po.phase_scratch + 8u * (std::size_t{po.phase_nx} + po.phase_ny); // twiddles and tables in front of the scratch
            po.row_band = false;
        }

        // --beam-hardening C1:C2[:C3[:C4]] as typed; refuses anything but two to four numbers
        inline auto parse_beam_hardening(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--beam-hardening C1:C2[:C3[:C4]]", v);
            const auto field = colon_fields(v);
            if(field.size() < 2u || field.size() > PARIS_HIP_BH_DEGREE_MAX)
                throw bad;
            po.bh = paris_hip_beam_hardening{};
            po.bh.degree = static_cast<std::uint32_t>(field.size());
            for(std::size_t k = 0; k < field.size(); ++k)
                po.bh.c[k] = read_number<float>(field[k], bad);
            po.beam_hardening = true;
        }

        // --fit-beam-hardening N[:SLICES[:MARGIN]] as typed; refuses anything but one to three unsigned numbers
        inline auto parse_fit_beam_hardening(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--fit-beam-hardening N[:SLICES[:MARGIN]]", v);
            const auto field = colon_fields(v);
            if(field.size() > 3u)
                throw bad;
            std::uint32_t value[3] = {0u, 32u, 2u};
            for(std::size_t k = 0; k < field.size(); ++k)
                value[k] = read_unsigned(field[k], bad);
            po.bh = paris_hip_beam_hardening{};
            po.bh.degree = value[0];
            po.bh_slices = value[1];
            po.bh_margin = value[2];
            po.fit_beam_hardening = true;
        }

        // --beam-hardening / --fit-beam-hardening: checked here, before any device work. The fit's pre-pass reads whole frames of the
        // detector the reconstruction sees: it has no full-width slots to bin from, so --bin is refused with it.
        inline auto check_beam_hardening(const program_options& po) -> void
        {
            if(po.beam_hardening && po.fit_beam_hardening)
                throw stage_construction_error{"--beam-hardening and --fit-beam-hardening cannot be combined: give the coefficients or have them fitted"};
            if(po.beam_hardening && paris_hip_beam_hardening_check(&po.bh) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--beam-hardening C1:C2[:C3[:C4]]: every coefficient must be finite"};
            if(!po.fit_beam_hardening)
                return;
            if(po.bh.degree < 1u || po.bh.degree > PARIS_HIP_BH_DEGREE_MAX || po.bh_slices < 1u || po.bh_margin > PARIS_HIP_BH_MARGIN_MAX)
                throw stage_construction_error{"--fit-beam-hardening N[:SLICES[:MARGIN]]: N must lie in 1 .. 4, SLICES must be at least 1 and MARGIN in 0 .. 4 (got "
                                               + std::to_string(po.bh.degree) + ":" + std::to_string(po.bh_slices) + ":" + std::to_string(po.bh_margin) + ")"};
            if(po.bh_slices < 2u * po.bh_margin + 1u)
                throw stage_construction_error{"--fit-beam-hardening: " + std::to_string(po.bh_slices) + " slice(s) hold no voxel with a margin of "
                                               + std::to_string(po.bh_margin) + " on both sides"};
            if(po.binning())
                throw stage_construction_error{"--fit-beam-hardening cannot be combined with --bin: its pre-pass reads the frames at the detector's size"};
            if(po.axis_only)
                throw stage_construction_error{"--fit-beam-hardening cannot be combined with --axis-only: nothing would be fitted"};
        }

        // --metal THR[:GROW[:MIN_PATH]] as typed; refuses anything but one to three numbers (the ranges: check_metal)
        inline auto parse_metal(const std::string& v, program_options& po) -> void
        {
            const auto usage = std::string{"--metal THR[:GROW[:MIN_PATH]]"};
            const auto bad = cannot_read(usage, v);
            const auto field = colon_fields(v);
            if(field.size() > 3u)
                throw bad;
            po.metal_threshold = read_number<float>(field[0], bad);
            if(field.size() > 1u)
            {
                const float g = read_number<float>(field[1], bad);
                if(!(g >= 0.f) || g != std::floor(g) || g > 1e6f)
                    throw bad;
                po.metal_grow = static_cast<std::uint32_t>(g);
            }
            if(field.size() > 2u)
            {
                po.metal_min_path = read_number<float>(field[2], bad);
                if(!(po.metal_min_path >= 0.f)) // (a negative or NaN MIN_PATH must not pass for "not given")
                    throw stage_construction_error{usage + ": MIN_PATH must be finite and not negative (got " + field[2] + ")"};
            }
            po.metal = true;
        }

        // --metal: checked here, before any device work. The metal outside a region of interest still casts a trace, and the list is
        // indexed in the whole grid: --roi is refused with it.
        inline auto check_metal(const program_options& po) -> void
        {
            if(!po.metal)
                return;
            if(po.enable_roi)
                throw stage_construction_error{"--metal cannot be combined with --roi: metal outside the region still casts a trace"};
            if(!std::isfinite(po.metal_threshold))
                throw stage_construction_error{"--metal THR[:GROW[:MIN_PATH]]: THR must be finite"};
            if(po.metal_grow > PARIS_HIP_METAL_GROW_MAX)
                throw stage_construction_error{"--metal THR[:GROW[:MIN_PATH]]: GROW must lie in 0 .. " + std::to_string(PARIS_HIP_METAL_GROW_MAX) + " (got "
                                               + std::to_string(po.metal_grow) + ")"};
            if(po.metal_min_path >= 0.f && !std::isfinite(po.metal_min_path))
                throw stage_construction_error{"--metal THR[:GROW[:MIN_PATH]]: MIN_PATH must be finite and not negative"};
            if(po.axis_only || po.roll_only)
                throw stage_construction_error{"--metal cannot be combined with --axis-only or --roll-only: nothing would be reconstructed"};
        }

        // --denoise SIGMA_R[:SIGMA_S[:RADIUS]] as typed; refuses anything but one or two numbers and an unsigned integer (the ranges:
        // check_denoise). Without RADIUS it is min(3, ceil(2 SIGMA_S)), at least 1 -- 0 for a SIGMA_S the check refuses anyway.
        inline auto parse_denoise(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--denoise SIGMA_R[:SIGMA_S[:RADIUS]]", v);
            const auto field = colon_fields(v);
            if(field.size() > 3u)
                throw bad;
            auto& s = po.denoise_setting;
            s.sigma_r = read_number<float>(field[0], bad);
            s.sigma_s = field.size() > 1u ? read_number<float>(field[1], bad) : 1.f;
            po.denoise_radius_given = field.size() > 2u;
            if(po.denoise_radius_given)
                s.radius = read_unsigned(field[2], bad);
            else if(std::isfinite(s.sigma_s) && s.sigma_s > 0.f)
                s.radius = static_cast<std::uint32_t>(std::min(3.0, std::max(1.0, std::ceil(2.0 * static_cast<double>(s.sigma_s)))));
            else
                s.radius = 0u;
            po.denoise = true;
        }

        // --denoise: checked here, before any device work and before the output directory is made
        inline auto check_denoise(const program_options& po) -> void
        {
            if(!po.denoise)
                return;
            const auto usage = std::string{"--denoise SIGMA_R[:SIGMA_S[:RADIUS]]"};
            const auto& s = po.denoise_setting;
            if(!std::isfinite(s.sigma_r) || !(s.sigma_r > 0.f))
                throw stage_construction_error{usage + ": SIGMA_R must be finite and greater than 0"};
            if(!std::isfinite(s.sigma_s) || !(s.sigma_s > 0.f))
                throw stage_construction_error{usage + ": SIGMA_S must be finite and greater than 0"};
            if(s.radius < 1u || s.radius > PARIS_HIP_BILATERAL_RADIUS_MAX)
                throw stage_construction_error{usage + ": RADIUS must lie in 1 .. " + std::to_string(PARIS_HIP_BILATERAL_RADIUS_MAX) + " (got "
                                               + std::to_string(s.radius) + ")"};
            if(paris_hip_volume_bilateral_check(&s) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{usage + ": SIGMA_R is too small for the range table (1024 / (4 SIGMA_R) is not a finite float)"};
            if(po.axis_only || po.roll_only)
                throw stage_construction_error{"--denoise cannot be combined with --axis-only or --roll-only: nothing would be written"};
        }

        // --find-axis LO:HI[:STEP] as typed; refuses anything but two or three numbers
        inline auto parse_find_axis(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--find-axis LO:HI[:STEP]", v);
            const auto field = colon_fields(v);
            if(field.size() < 2u || field.size() > 3u)
                throw bad;
            po.axis_lo = read_number<float>(field[0], bad);
            po.axis_hi = read_number<float>(field[1], bad);
            po.axis_step = field.size() > 2u ? read_number<float>(field[2], bad) : 0.25f;
            po.find_axis = true;
        }

        inline auto parse_axis_rows(const std::string& v, program_options& po) -> void
        {
            po.axis_rows = read_unsigned(v, cannot_read("--axis-rows R", v));
            po.axis_rows_given = true;
        }

        // --find-axis: the candidates, the scan and the setting are checked for this detector here, before any device work. The
        // search needs a full, equidistant circle: it is refused with --short-scan, with an angle file, and for frames (after the
        // quality stride) whose count times their angle step differs from 360 degrees by more than half a step
        inline auto check_axis(program_options& po) -> void
        {
            if(!po.find_axis)
            {
                if(po.axis_only || po.axis_rows_given)
                    throw stage_construction_error{"--axis-rows and --axis-only need --find-axis"};
                return;
            }
            if(po.short_scan)
                throw stage_construction_error{"--find-axis needs a full circle: it cannot be combined with --short-scan"};
            if(po.enable_angles)
                throw stage_construction_error{"--find-axis needs equidistant projections: it cannot be combined with an angle file (--angles)"};
            const double span = static_cast<double>(po.axis_hi) - static_cast<double>(po.axis_lo);
            if(!std::isfinite(po.axis_lo) || !std::isfinite(po.axis_hi) || !std::isfinite(po.axis_step) || !(po.axis_step > 0.f) || !(span >= 0.0)
               || span / static_cast<double>(po.axis_step) > 1023.0)
                throw stage_construction_error{"--find-axis LO:HI[:STEP]: LO <= HI and STEP > 0, all finite, and at most 1024 candidates (got "
                                               + std::to_string(po.axis_lo) + ":" + std::to_string(po.axis_hi) + ":" + std::to_string(po.axis_step) + ")"};
            po.axis_count = static_cast<std::uint32_t>(std::floor(span / static_cast<double>(po.axis_step) + 0.5)) + 1u;
            const auto a = frame_angles(po.input_path, false, po.angle_path, po.quality, po.det_geo.delta_phi);
            const double step = a.size() >= 2u ? static_cast<double>(a[1]) - static_cast<double>(a[0]) : 0.0;
            if(a.size() < 4u || !(step > 0.0) || std::abs(static_cast<double>(a.size()) * step - 360.0) > 0.5 * step)
            {
                char msg[256];
                std::snprintf(msg, sizeof msg, "--find-axis needs a full circle of at least 4 projections at a positive angle step: %zu projection(s) "
                              "%.6g degrees apart cover %.6g degrees", a.size(), step, static_cast<double>(a.size()) * step);
                throw stage_construction_error{msg};
            }
            po.axis_frames = static_cast<std::uint32_t>(a.size());
            const auto search = paris_hip_axis_search{po.axis_lo, po.axis_step, po.axis_count, po.axis_rows, 0u};
            const int rc = paris_hip_axis_search_check(&search, &po.det_geo, po.axis_frames, nullptr, nullptr);
            if(rc == PARIS_HIP_ERROR_UNSUPPORTED)
                throw stage_construction_error{"--find-axis: the candidates times the detector's columns, or the sinogram, exceed 2^32 - 1 entries"};
            if(rc != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--find-axis / --axis-rows: R must lie in 1 .. 64 and within the detector's " + std::to_string(po.det_geo.n_col)
                                               + " rows, and the geometry needs a positive pixel size and source distance (got R = "
                                               + std::to_string(po.axis_rows) + ")"};
        }

        // --detector-roll DEG as typed
        inline auto parse_detector_roll(const std::string& v, program_options& po) -> void
        {
            po.roll_deg = read_number<float>(v, cannot_read("--detector-roll DEG", v));
            po.roll = true;
        }

        // --find-roll LO:HI[:STEP] as typed; refuses anything but two or three numbers
        inline auto parse_find_roll(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--find-roll LO:HI[:STEP]", v);
            const auto field = colon_fields(v);
            if(field.size() < 2u || field.size() > 3u)
                throw bad;
            po.roll_lo = read_number<float>(field[0], bad);
            po.roll_hi = read_number<float>(field[1], bad);
            po.roll_step = field.size() > 2u ? read_number<float>(field[2], bad) : 0.25f;
            po.find_roll = true;
        }

        // --detector-roll / --find-roll: the angle, the candidates and the scan are checked for this detector here, before any device
        // work. The search needs a full, equidistant circle on a centred detector: it is refused with --short-scan, with
        // --offset-detector, with an angle file, and for frames (after the quality stride) that do not cover 360 degrees
        inline auto check_roll(program_options& po) -> void
        {
            if(po.roll_only && !po.find_roll)
                throw stage_construction_error{"--roll-only needs --find-roll"};
            if(po.roll && po.find_roll)
                throw stage_construction_error{"--detector-roll and --find-roll cannot be combined: give the angle or have it found"};
            if((po.roll || po.find_roll) && po.fit_beam_hardening)
                throw stage_construction_error{"--detector-roll / --find-roll cannot be combined with --fit-beam-hardening: its pre-pass does not resample the frames"};
            if(po.roll)
            {
                const auto setting = paris_hip_detector_roll{po.roll_deg};
                if(paris_hip_detector_roll_check(&setting, &po.det_geo) != PARIS_HIP_SUCCESS)
                    throw stage_construction_error{"--detector-roll DEG: DEG must be finite, not 0 and at most 10 in size, on a detector of at least 2 x 2 pixels "
                                                   "with positive pixel sizes (got " + std::to_string(po.roll_deg) + ")"};
            }
            if(!po.find_roll)
                return;
            if(po.short_scan)
                throw stage_construction_error{"--find-roll needs a full circle: it cannot be combined with --short-scan"};
            if(po.offset_detector)
                throw stage_construction_error{"--find-roll needs a centred detector: it cannot be combined with --offset-detector"};
            if(po.enable_angles)
                throw stage_construction_error{"--find-roll needs equidistant projections: it cannot be combined with an angle file (--angles)"};
            if(po.roll_only && po.axis_only)
                throw stage_construction_error{"--roll-only cannot be combined with --axis-only: the run would stop before the roll search"};
            const double span = static_cast<double>(po.roll_hi) - static_cast<double>(po.roll_lo);
            if(!std::isfinite(po.roll_lo) || !std::isfinite(po.roll_hi) || !std::isfinite(po.roll_step) || !(po.roll_step > 0.f) || !(span >= 0.0)
               || span / static_cast<double>(po.roll_step) > 255.0)
                throw stage_construction_error{"--find-roll LO:HI[:STEP]: LO <= HI and STEP > 0, all finite, and at most 256 candidates (got "
                                               + std::to_string(po.roll_lo) + ":" + std::to_string(po.roll_hi) + ":" + std::to_string(po.roll_step) + ")"};
            po.roll_count = static_cast<std::uint32_t>(std::floor(span / static_cast<double>(po.roll_step) + 0.5)) + 1u;
            const auto a = frame_angles(po.input_path, false, po.angle_path, po.quality, po.det_geo.delta_phi);
            const double step = a.size() >= 2u ? static_cast<double>(a[1]) - static_cast<double>(a[0]) : 0.0;
            if(a.size() < 4u || !(step > 0.0) || std::abs(static_cast<double>(a.size()) * step - 360.0) > 0.5 * step)
            {
                char msg[256];
                std::snprintf(msg, sizeof msg, "--find-roll needs a full circle of at least 4 projections at a positive angle step: %zu projection(s) "
                              "%.6g degrees apart cover %.6g degrees", a.size(), step, static_cast<double>(a.size()) * step);
                throw stage_construction_error{msg};
            }
            const auto search = paris_hip_roll_search{po.roll_lo, po.roll_step, po.roll_count, 0u};
            if(paris_hip_roll_search_check(&search, &po.det_geo, nullptr, nullptr, nullptr) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--find-roll LO:HI[:STEP]: every candidate must lie within 10 degrees of 0 and leave pixels inside the margins "
                                               "of the detector (got " + std::to_string(po.roll_lo) + ":" + std::to_string(po.roll_hi) + ":"
                                               + std::to_string(po.roll_step) + ")"};
        }

        // --lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]] as typed; refuses anything but one to four pairs of numbers
        inline auto parse_lag(const std::string& v, program_options& po) -> void
        {
            const auto bad = cannot_read("--lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]]", v);
            const auto field = colon_fields(v);
            if(field.size() % 2u != 0u || field.size() > 2u * PARIS_HIP_LAG_TERMS_MAX)
                throw bad;
            po.lag_model.terms = static_cast<std::uint32_t>(field.size() / 2u);
            for(std::size_t k = 0; k < field.size(); ++k)
            {
                const float x = read_number<float>(field[k], bad);
                (k % 2u == 0u ? po.lag_model.b : po.lag_model.a)[k / 2u] = x;
            }
            po.lag = true;
        }

        inline auto parse_lag_start(const std::string& v, program_options& po) -> void
        {
            if(v == "rest") po.lag_model.start = PARIS_HIP_LAG_START_REST;
            else if(v == "steady") po.lag_model.start = PARIS_HIP_LAG_START_STEADY;
            else throw stage_construction_error{"--lag-start rest|steady: unknown start " + v};
            po.lag_start_given = true;
        }

        // --lag / --lag-start: checked here, before any device work. The correction works on counts, so it needs --flat; and on every
        // frame the detector took, so --quality above 1 is refused: the skipped frames still fed the detector's memory.
        inline auto check_lag(const program_options& po) -> void
        {
            if(!po.lag)
            {
                if(po.lag_start_given)
                    throw stage_construction_error{"--lag-start needs --lag"};
                return;
            }
            if(po.flat_path.empty())
                throw stage_construction_error{"--lag needs --flat: the lag correction works on detector counts, before the dark / flat correction"};
            if(po.quality > 1u)
                throw stage_construction_error{"--lag cannot be combined with --quality " + std::to_string(po.quality)
                                               + ": the skipped frames still fed the detector's memory"};
            if(paris_hip_lag_model_check(&po.lag_model) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]]: every weight B and decay rate per frame A must be finite and above 0, "
                                               "and b_0 = 1 - sum B / (1 - exp(-A)) must be above 0"};
        }

        // --offset-detector: refused here, before any device work, together with --short-scan (that combination needs a different
        // weight), for a detector whose overlap tau = (n_row / 2 - |delta_s|) l_px_row is below 2 pixels, and unless the frames of the
        // run (after the quality stride) have monotonic angles whose span plus one mean step reaches 360 degrees within half a step
        inline auto check_offset_detector(const program_options& po) -> void
        {
            if(po.short_scan)
                throw stage_construction_error{"--offset-detector and --short-scan together: a short scan with an offset detector needs a "
                                               "different weight"};
            float gamma_tau = 0.f;
            if(paris_hip_offset_detector_check(&po.det_geo, &gamma_tau) != PARIS_HIP_SUCCESS)
            {
                char msg[256];
                std::snprintf(msg, sizeof msg, "--offset-detector: the overlap tau = (n_row / 2 - |delta_s|) = %.4f pixels (n_row %u, delta_s %.4f); "
                              "the weight needs at least 2", static_cast<double>(po.det_geo.n_row) / 2.0 - std::abs(static_cast<double>(po.det_geo.delta_s)),
                              po.det_geo.n_row, static_cast<double>(po.det_geo.delta_s));
                throw stage_construction_error{msg};
            }
            const auto a = frame_angles(po.input_path, po.enable_angles, po.angle_path, po.quality, po.det_geo.delta_phi);
            if(a.size() < 2u)
                throw stage_construction_error{"--offset-detector needs at least two projections"};
            const bool up = a[1] > a[0];
            for(std::size_t i = 1; i < a.size(); ++i)
                if(up ? !(a[i] > a[i - 1]) : !(a[i] < a[i - 1]))
                    throw stage_construction_error{"--offset-detector: the projection angles are not monotonic (frame " + std::to_string(i) + ": "
                                                   + std::to_string(a[i]) + " degrees after " + std::to_string(a[i - 1]) + ")"};
            const double span = std::abs(static_cast<double>(a.back()) - static_cast<double>(a.front()));
            const double step = span / static_cast<double>(a.size() - 1u);
            if(360.0 - (span + step) > step / 2.0)
            {
                char msg[256];
                std::snprintf(msg, sizeof msg, "--offset-detector: the projections cover %.4f degrees (%.4f plus one step of %.4f), an offset "
                              "detector needs a full circle of 360", span + step, span, step);
                throw stage_construction_error{msg};
            }
        }

        // The options whose value a parse_* reads, by flag: paris.hip's command line and demo/paris_hip_options look them up here
        // (nullptr: the flag is not one of them). Flags without a value, and the values main() converts itself, are main()'s own.
        using option_parser = void (*)(const std::string&, program_options&);
        inline auto find_option_parser(const std::string& flag) -> option_parser
        {
            static const struct
            {
                const char* flag;
                option_parser parse;
            } table[] = {
                {"--zingers", parse_zingers},
                {"--zinger-polarity", parse_zinger_polarity},
                {"--extend-rows", parse_extend_rows},
                {"--rings", parse_rings},
                {"--bin", parse_bin},
                {"--find-axis", parse_find_axis},
                {"--axis-rows", parse_axis_rows},
                {"--detector-roll", parse_detector_roll},
                {"--find-roll", parse_find_roll},
                {"--air-region", parse_air_region},
                {"--starvation", parse_starvation},
                {"--scatter", parse_scatter},
                {"--scatter-iterations", parse_scatter_iterations},
                {"--scatter-limit", parse_scatter_limit},
                {"--scatter-margin", parse_scatter_margin},
                {"--phase", [](const std::string& v, program_options& po) { parse_phase(v, po, true); }},
                {"--phase-alpha", [](const std::string& v, program_options& po) { parse_phase(v, po, false); }},
                {"--phase-floor", parse_phase_floor},
                {"--beam-hardening", parse_beam_hardening},
                {"--fit-beam-hardening", parse_fit_beam_hardening},
                {"--lag", parse_lag},
                {"--lag-start", parse_lag_start},
                {"--metal", parse_metal},
                {"--denoise", parse_denoise},
                {"--voxel-type", parse_voxel_type},
                {"--voxel-range", parse_voxel_range},
            };
            for(const auto& entry : table)
                if(flag == entry.flag)
                    return entry.parse;
            return nullptr;
        }
    }
}

#endif

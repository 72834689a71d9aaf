// paris.hip -- command-line reconstruction with the MI355X backend: HIS projections in, one DDBVF volume out.
// Options carry the reference's names (src/program_options.cpp:46-78); parsing is deliberately minimal (the
// reference's Boost.Program_options front end is out of scope).
//
//   paris.hip --geometry geo.ini --input <dir> --output <dir> [--name vol] [--angles file] [--quality q]
//             [--roi --roi-x1 a --roi-x2 b --roi-y1 c --roi-y2 d --roi-z1 e --roi-z2 f]
//             [--slabs n] [--devices n] [--f16] [--no-row-band] [--batch n] [--drain-chunk-kib n] [--share-frames 0|1] [--one-volume] [--pipeline-slabs n] [--no-read-ahead]
//             [--window ramp|shepp-logan] [--short-scan] [--offset-detector] [--flat file.his [--dark file.his] [--min-transmission t]]
//             [--defects mask.raw] [--defects-from-flat] [--zingers ABS[:REL] [--zinger-polarity bright|dark|both]] [--rings H[:FLOOR[:LIMIT]]]
//             [--extend-rows W[:M]] [--voxel-type u8|u16 --voxel-range LO:HI|auto[:P_LO:P_HI]] [--bin BX[:BY]]
//             [--find-axis LO:HI[:STEP] [--axis-rows R] [--axis-only]] [--air-region X0:Y0:W:H[:LIMIT]]
//             [--beam-hardening C1:C2[:C3[:C4]] | --fit-beam-hardening N[:SLICES[:MARGIN]]]
//             [--lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]] [--lag-start rest|steady]]
//             [--metal THR[:GROW[:MIN_PATH]]] [--phase DELTA_BETA:ENERGY_KEV[:MARGIN] | --phase-alpha MM2[:MARGIN]] [--phase-floor T]
//             [--scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2] [--scatter-iterations N] [--scatter-limit F] [--scatter-margin M]]
//             [--denoise SIGMA_R[:SIGMA_S[:RADIUS]]] [--starvation P0[:GAIN[:RADIUS]]]
// geo.ini: key=value lines for n_row n_col l_px_row l_px_col delta_s delta_t d_so d_od delta_phi (:83-91).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>

#include "paris/reconstruct.h"

namespace
{
    auto parse_geometry(const std::string& path) -> paris::detector_geometry
    {
        auto file = std::ifstream{path};
        if(!file)
            throw paris::stage_construction_error{"cannot open geometry file " + path};
        auto kv = std::map<std::string, std::string>{};
        auto line = std::string{};
        while(std::getline(file, line))
        {
            const auto hash = line.find('#');
            if(hash != std::string::npos)
                line.erase(hash);
            const auto eq = line.find('=');
            if(eq == std::string::npos)
                continue;
            auto trim = [](std::string s) {
                const auto b = s.find_first_not_of(" \t\r");
                const auto e = s.find_last_not_of(" \t\r");
                return b == std::string::npos ? std::string{} : s.substr(b, e - b + 1);
            };
            kv[trim(line.substr(0, eq))] = trim(line.substr(eq + 1));
        }
        auto need = [&](const char* k) -> const std::string& {
            auto it = kv.find(k);
            if(it == kv.end())
                throw paris::stage_construction_error{std::string{"the option '"} + k + "' is required but missing"};
            return it->second;
        };
        auto g = paris::detector_geometry{};
        g.n_row = static_cast<std::uint32_t>(std::stoul(need("n_row")));
        g.n_col = static_cast<std::uint32_t>(std::stoul(need("n_col")));
        g.l_px_row = std::stof(need("l_px_row"));
        g.l_px_col = std::stof(need("l_px_col"));
        g.delta_s = std::stof(need("delta_s"));
        g.delta_t = std::stof(need("delta_t"));
        g.d_so = std::stof(need("d_so"));
        g.d_od = std::stof(need("d_od"));
        g.delta_phi = std::stof(need("delta_phi"));
        return g;
    }
}

int main(int argc, char** argv)
{
    try
    {
        auto po = paris::program_options{};
        auto geometry = std::string{};
        for(int a = 1; a < argc; ++a)
        {
            const auto k = std::string{argv[a]};
            auto val = [&]() -> std::string {
                if(a + 1 >= argc)
                    throw paris::stage_construction_error{"missing value for " + k};
                return argv[++a];
            };
            if(k == "--help" || k == "-h")
            {
                std::printf("paris.hip --geometry geo.ini --input <dir of .his files> --output <dir> [--name vol] [--angles file] [--quality q]\n"
                            "          [--roi --roi-x1 a --roi-x2 b --roi-y1 c --roi-y2 d --roi-z1 e --roi-z2 f]\n"
                            "          [--slabs n] [--devices n] [--f16] [--window ramp|shepp-logan] [--batch n] [--no-row-band] [--share-frames 0|1] [--one-volume] [--pipeline-slabs n] [--no-read-ahead]\n"
                            "          [--drain-chunk-kib n] [--short-scan] [--offset-detector] [--flat file.his [--dark file.his] [--min-transmission t]]\n"
                            "          [--defects mask.raw] [--defects-from-flat] [--zingers ABS[:REL] [--zinger-polarity bright|dark|both]]\n"
                            "          [--rings H[:FLOOR[:LIMIT]]]\n"
                            "          [--extend-rows W[:M]] [--voxel-type u8|u16 --voxel-range LO:HI|auto[:P_LO:P_HI]] [--bin BX[:BY]]\n"
                            "          [--find-axis LO:HI[:STEP] [--axis-rows R] [--axis-only]] [--air-region X0:Y0:W:H[:LIMIT]]\n"
                            "          [--beam-hardening C1:C2[:C3[:C4]] | --fit-beam-hardening N[:SLICES[:MARGIN]]]\n"
                            "          [--detector-roll DEG | --find-roll LO:HI[:STEP] [--roll-only]]\n"
                            "          [--lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]] [--lag-start rest|steady]]\n"
                            "          [--metal THR[:GROW[:MIN_PATH]]] [--phase DELTA_BETA:ENERGY_KEV[:MARGIN] | --phase-alpha MM2[:MARGIN]] [--phase-floor T]\n"
                            "          [--scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2] [--scatter-iterations N] [--scatter-limit F] [--scatter-margin M]]\n"
                            "          [--denoise SIGMA_R[:SIGMA_S[:RADIUS]]] [--starvation P0[:GAIN[:RADIUS]]]\n"
                            "geo.ini: key=value lines for n_row n_col l_px_row l_px_col delta_s delta_t d_so d_od delta_phi\n"
                            "Reconstructs the HIS projections of <dir> (sorted by path) into <output>/<name>.ddbvf on all MI355X of the node.\n"
                            "--short-scan: the projections form a short scan from their first to their last angle (at least 180 degrees plus\n"
                            "twice the fan angle); each is weighted by Parker's redundancy weight before the cosine weight.\n"
                            "--offset-detector: the detector is shifted sideways (delta_s) over a full circle (half fan); each projection is\n"
                            "weighted by the offset-detector redundancy weight before the cosine weight.\n"
                            "--flat / --dark: the projections are detector counts; each is corrected with the mean flat (and dark) frame of\n"
                            "these HIS files to line integrals -ln(max((I - D) / (F - D), t)) on the device, t = --min-transmission (1e-5).\n"
                            "--defects: n_col x n_row raw bytes, nonzero = defective pixel; --defects-from-flat: the pixels whose flat is not above\n"
                            "their dark as well (needs --flat). Each defective pixel is replaced on the device, after the correction and before\n"
                            "the weights, by the inverse-square-distance weighted mean of the good pixels on the nearest ring that holds one.\n"
                            "--zingers: every pixel that differs from the median m of its 3 x 3 window by more than ABS + REL * |m| is replaced by\n"
                            "m on the device, after the repair and before the weights -- pixels above m (bright: the default), below it (dark: the\n"
                            "default with --flat) or both; a frame with more flagged pixels than 1/256 of the detector (1024 at least) is left as it is.\n"
                            "--rings: stationary detector offsets, which reconstruct to rings. The scan is read once before the reconstruction;\n"
                            "every pixel's mean over the views is compared with the running median of 2 H + 1 pixels (H in 1 .. 32) along its\n"
                            "detector row, and a difference c with FLOOR <= |c| (and |c| <= LIMIT unless LIMIT is 0; both default to 0) is\n"
                            "subtracted from every frame on the device, after the zinger filter and before the weights.\n"
                            "--extend-rows: the object is wider than the detector (truncated rows). The row filter acts as if every row went on\n"
                            "beyond either edge as the mean of its M outermost pixels (1, 2, 4 or 8; default 4) times a cos^2 taper of W pixels\n"
                            "(1 .. 16384; 16 is a good start, longer is not better) instead of dropping to 0.\n"
                            "--voxel-type / --voxel-range: the voxels are written as 8- or 16-bit integers over the grey window [LO, HI], quantised\n"
                            "on the device, into <output>/<name>.raw with the MetaImage header <name>.mhd beside it, instead of the float DDBVF.\n"
                            "auto: the window between the percentiles P_LO and P_HI (0.1 and 99.9) of the finished volume's 4096-bin histogram;\n"
                            "needs --slabs 1 on one device.\n"
                            "--bin: the detector is read as bins of BX x BY pixels (each 1, 2, 4 or 8; BY defaults to BX): every frame is uploaded as\n"
                            "stored and binned on the device before the correction, each binned pixel the mean of its pixels that --defects (and\n"
                            "--defects-from-flat) do not mark; the dark, the flat and the defect map are binned alike, and the geometry -- and with\n"
                            "it the volume -- is the binned detector's.\n"
                            "--find-axis: delta_s, the horizontal offset of the rotation axis, is found from the scan itself and replaces the\n"
                            "geometry file's. The projections must form a full circle at equal steps (no --short-scan, no --angles). The scan is\n"
                            "read once before the reconstruction (together with --rings when both are given; alone, only the rows it needs): the\n"
                            "R rows (--axis-rows, 1 .. 64, default 2) about the mid-plane are summed into a sinogram, and each candidate LO,\n"
                            "LO + STEP .. HI [pixels; binned pixels with --bin; STEP defaults to 0.25, at most 1024 candidates] is scored on the\n"
                            "device by the mean squared difference between every sample and its conjugate ray half a turn away. The estimate is\n"
                            "the minimum of a parabola through the best candidate and its neighbours. --axis-only prints it and stops.\n"
                            "--air-region: the source's output drifts from frame to frame while the flat was taken once. Columns X0 .. X0 + W - 1,\n"
                            "rows Y0 .. Y0 + H - 1 of the frame [binned pixels with --bin; at most 2^20 pixels] see only air in every view: the\n"
                            "mean line integral of the rectangle's pixels (those --defects marks and values that are not finite left out) is\n"
                            "subtracted from the whole frame on the device, directly after the correction and before the repair. A frame with\n"
                            "fewer than half the rectangle's pixels left, or whose mean exceeds LIMIT in size (0, the default: no limit), stays\n"
                            "as it is and is counted.\n"
                            "--beam-hardening: a polychromatic tube makes the line integral concave in the path length, and the volume of a\n"
                            "homogeneous part comes out cupped. Every line integral p >= 0 becomes C1 p + C2 p^2 [+ C3 p^3 [+ C4 p^4]] on the\n"
                            "device, after the ring correction and before every weight; a negative p (noise in air) becomes C1 p.\n"
                            "--fit-beam-hardening: the coefficients C1 .. CN (N in 1 .. 4) are found from the scan itself. The scan is read once\n"
                            "before the reconstruction (after the pre-pass of --rings and --find-axis, whose results it uses): p, p^2 .. p^N are\n"
                            "each reconstructed into the central SLICES slices of the volume (default 32), the slices are split into object and\n"
                            "air by Otsu's threshold, leaving out every voxel within MARGIN voxels (0 .. 4, default 2) of the other class, and the\n"
                            "combination that is flattest over both is solved for. One material only; not with --bin or --beam-hardening.\n"
                            "--detector-roll: the detector is rotated in its own plane by DEG degrees (not 0, at most 10 in size). Every frame is\n"
                            "resampled on the device, bilinearly with the edge replicated, onto a detector whose rows are perpendicular to the\n"
                            "projected rotation axis -- a rotation in millimetres about the axis column and the centre row -- after the\n"
                            "beam-hardening correction and before every weight.\n"
                            "--find-roll: DEG is found from the scan itself. The projections must form a full circle at equal steps on a centred\n"
                            "detector (no --short-scan, no --offset-detector, no --angles). The scan is read once before the reconstruction\n"
                            "(together with --rings and --find-axis when given, after the axis search, whose delta_s it uses): the mean of all\n"
                            "frames is mirror-symmetric about the projected axis in every detector row, and each candidate LO, LO + STEP .. HI\n"
                            "[degrees; STEP defaults to 0.25, at most 256 candidates] is scored on the device by the mean squared asymmetry of\n"
                            "the mean frame rolled back by it. The estimate is the minimum of a parabola through the best candidate and its\n"
                            "neighbours. --roll-only prints it and stops. Not with --fit-beam-hardening.\n"
                            "--lag: an a-Si flat panel carries a few per cent of every frame's signal over into the following frames. Its impulse\n"
                            "response is b_0 at once plus one to four terms B_n exp(-A_n k), k frames later (B_n, A_n > 0; b_0 = 1 - sum B_n /\n"
                            "(1 - exp(-A_n)) must stay above 0). Every frame's counts are deconvolved recursively on the device, in the order of the\n"
                            "files, after the upload (and --bin) and before the dark / flat correction; each pass over the scan starts from frame 0.\n"
                            "--lag-start steady (the default): the beam was on and the first view had been seen for a long time; rest: the detector\n"
                            "had seen nothing. Needs --flat (the frames must be counts); not with --quality above 1 (the skipped frames still fed\n"
                            "the detector's memory).\n"
                            "--metal: metal (a screw, a pin, a filling) drives its rays to the detector's floor and the ramp filter spreads the\n"
                            "error as streaks. A pre-pass on the first device, after every other pre-pass, reconstructs the whole volume once,\n"
                            "takes the voxels above THR [the volume's own units] out of it, forward-projects their mask and marks every pixel\n"
                            "whose ray crosses more than MIN_PATH mm of it [default: half the smallest voxel edge], widened by GROW pixels [0 .. 4,\n"
                            "default 1]. In the reconstruction those pixels of every frame are replaced by linear interpolation along the row,\n"
                            "after the roll and before the weights, and every slab gets its metal voxels back. The pre-pass needs the whole\n"
                            "volume on one device. Not with --roi.\n"
                            "--denoise: the finished volume passes an edge-preserving 3-D bilateral filter on the device before it is written (or\n"
                            "quantised: --voxel-type and its auto window then see the filtered voxels). A voxel becomes the mean of its\n"
                            "(2 RADIUS + 1)^3 neighbours weighted by a Gaussian of their distance, SIGMA_S in VOXELS [default 1; the same along x, y\n"
                            "and z, whatever the voxel edges], times a Gaussian of their difference in value, SIGMA_R in the volume's own units;\n"
                            "neighbours further than 4 SIGMA_R in value count nothing. RADIUS is 1, 2 or 3 [default min(3, ceil(2 SIGMA_S))].\n"
                            "Slabs are reconstructed with RADIUS more slices on each side, so the file does not depend on --slabs, --devices or\n"
                            "--drain-chunk-kib. Runs after the metal reinsertion; with --roi the grid is the region's. Not with --axis-only or\n"
                            "--roll-only.\n"
                            "--starvation: along the longest or densest paths the detector counts a handful of photons, and the ramp filter turns\n"
                            "those noisy pixels into streaks. Every frame is smoothed on the device where its line integral lies above P0, by a 2-D\n"
                            "Gaussian over (2 RADIUS + 1)^2 pixels [RADIUS 1 .. 4, default 3] whose width grows with the excess over P0 so that the\n"
                            "noise comes down to that at P0 (GAIN scales the width, default 1; at most RADIUS / 2 pixels); pixels at or below P0 keep\n"
                            "their bits. After the ring correction, before the scatter correction; whole frames (planned as --no-row-band). Not\n"
                            "with --axis-only or --roll-only.\n");
                return 0;
            }
            if(k == "--geometry") geometry = val();
            else if(k == "--input") po.input_path = val();
            else if(k == "--output") po.output_path = val();
            else if(k == "--name") po.prefix = val();
            else if(k == "--angles") { po.angle_path = val(); po.enable_angles = true; }
            else if(k == "--quality") po.quality = static_cast<std::uint16_t>(std::stoul(val()));
            else if(k == "--roi") po.enable_roi = true;
            else if(k == "--roi-x1") po.roi.x1 = static_cast<std::uint32_t>(std::stoul(val()));
            else if(k == "--roi-x2") po.roi.x2 = static_cast<std::uint32_t>(std::stoul(val()));
            else if(k == "--roi-y1") po.roi.y1 = static_cast<std::uint32_t>(std::stoul(val()));
            else if(k == "--roi-y2") po.roi.y2 = static_cast<std::uint32_t>(std::stoul(val()));
            else if(k == "--roi-z1") po.roi.z1 = static_cast<std::uint32_t>(std::stoul(val()));
            else if(k == "--roi-z2") po.roi.z2 = static_cast<std::uint32_t>(std::stoul(val()));
            else if(k == "--slabs") po.slabs = std::stoi(val());
            else if(k == "--devices") po.devices = std::stoi(val());
            else if(k == "--f16") po.f16 = true;
            else if(k == "--short-scan") po.short_scan = true;
            else if(k == "--offset-detector") po.offset_detector = true;
            else if(k == "--flat") po.flat_path = val();
            else if(k == "--dark") po.dark_path = val();
            else if(k == "--min-transmission") po.t_min = std::stof(val());
            else if(k == "--defects") po.defects_path = val();
            else if(k == "--defects-from-flat") po.defects_from_flat = true;
            else if(k == "--axis-only") po.axis_only = true;
            else if(k == "--roll-only") po.roll_only = true;
            else if(k == "--no-row-band") po.row_band = false;
            else if(k == "--window")
            {
                const auto w = val();
                if(w == "ramp") po.window = PARIS_HIP_WINDOW_RAMP;
                else if(w == "shepp-logan") po.window = PARIS_HIP_WINDOW_SHEPP_LOGAN;
                else throw paris::stage_construction_error{"unknown filter window " + w};
            }
            else if(k == "--batch") po.batch = std::stoi(val());
            else if(k == "--share-frames") po.share_frames = std::stoi(val());
            else if(k == "--one-volume") po.two_volumes = false;
            else if(k == "--no-read-ahead") po.read_ahead = false;
            else if(k == "--pipeline-slabs") po.pipeline_slabs = std::stoi(val());
            else if(k == "--drain-chunk-kib") po.drain_chunk_bytes = static_cast<std::size_t>(std::stoull(val())) << 10;
            else if(const auto parse = paris::detail::find_option_parser(k)) parse(val(), po); // the options paris/options.h reads
            else throw paris::stage_construction_error{"unknown option " + k};
        }
        if(geometry.empty())
            throw paris::stage_construction_error{"the option '--geometry' is required but missing"};
        po.det_geo = parse_geometry(geometry);
        if(po.input_path.empty() || po.output_path.empty()) // src/program_options.cpp:117-122: both or neither
        {
            const auto setting = paris_hip_binning{po.bin_x, po.bin_y};
            auto geo = po.det_geo;
            if(paris_hip_binned_geometry(&setting, &po.det_geo, &geo) != PARIS_HIP_SUCCESS)
                throw paris::stage_construction_error{"--bin: the detector does not hold one bin"};
            const auto v = paris::calculate_volume_geometry(geo);
            std::printf("Volume dimensions [vx]: %u x %u x %u, voxel size %.6g mm (no --input/--output: nothing to do)\n", v.dim_x, v.dim_y,
                        v.dim_z, v.l_vx_x);
            return 0;
        }
        po.enable_io = true;
        const auto r = paris::run(po);
        if(r.binning)
            std::printf("binning on: %u x %u bins, detector %u x %u -> %u x %u, %llu binned pixel(s) without a good source pixel marked defective\n",
                        r.bin_x, r.bin_y, r.src_row, r.src_col, r.binned_row, r.binned_col, static_cast<unsigned long long>(r.binned_defective));
        if(r.flat_frames != 0)
            std::printf("dark / flat correction on: %u flat frame(s), %u dark frame(s)%s, min transmission %g\n", r.flat_frames, r.dark_frames,
                        r.dark_frames == 0 ? " (zero dark)" : "", static_cast<double>(po.t_min));
        if(r.lag)
        {
            std::printf("lag correction on: %u term(s)", r.lag_model.terms);
            for(std::uint32_t n = 0; n < r.lag_model.terms; ++n)
                std::printf(" %.9g:%.9g", static_cast<double>(r.lag_model.b[n]), static_cast<double>(r.lag_model.a[n]));
            std::printf(", b_0 = %.6g, every pass over the scan starts %s\n", r.lag_b0,
                        r.lag_model.start == PARIS_HIP_LAG_START_STEADY ? "steady" : "at rest");
        }
        if(r.defect_map)
            std::printf("defect map on: %llu defective pixel(s), %llu unrepairable (no good pixel within %d)\n",
                        static_cast<unsigned long long>(r.defects.defects), static_cast<unsigned long long>(r.defects.unrepairable), PARIS_HIP_DEFECT_R_MAX);
        const auto air_line = [&](const char* where, const paris_hip_air_counts& c) {
            std::printf("air region %s: columns %u .. %u, rows %u .. %u of the %u x %u frame, %llu frame band(s) measured, %llu normalised, "
                        "%llu with too few pixels, %llu above the limit", where, po.air_region.x0, po.air_region.x0 + po.air_region.width - 1u,
                        po.air_region.y0, po.air_region.y0 + po.air_region.height - 1u, r.air_row, r.air_col,
                        static_cast<unsigned long long>(c.frames), static_cast<unsigned long long>(c.normalised),
                        static_cast<unsigned long long>(c.too_few), static_cast<unsigned long long>(c.above_limit));
            if(c.normalised != 0u)
                std::printf(", values %.6g .. %.6g", static_cast<double>(c.min_a), static_cast<double>(c.max_a));
            std::printf("\n");
            if(c.normalised != c.frames)
                std::printf("warning: %llu frame band(s) were not normalised %s: the air region holds too few good pixels, or the object reaches into it\n",
                            static_cast<unsigned long long>(c.frames - c.normalised), where);
        };
        if(po.air && (r.ring_filter || r.axis_search))
            air_line("in the pre-pass", r.air_prepass);
        if(r.air_region)
            air_line("on", r.air);
        if(r.row_extension)
            std::printf("row extension on: cos^2 taper of %u pixel(s), mean of %u edge pixel(s)\n", po.extend_taper, po.extend_edge);
        if(r.zinger_filter)
            std::printf("zinger filter on: %llu frame band(s) examined, %llu pixel(s) replaced, %llu saturated (left as they were)\n",
                        static_cast<unsigned long long>(r.zingers.frames), static_cast<unsigned long long>(r.zingers.replaced),
                        static_cast<unsigned long long>(r.zingers.saturated_frames));
        if(r.ring_filter)
            std::printf("ring filter on: %u frame(s) in the pre-pass (%.3f s), %llu pixel(s) corrected, %llu below the floor, %llu above the limit, "
                        "%llu not finite, largest |c| %.6g\n", r.ring_frames, r.ring_prepass_s, static_cast<unsigned long long>(r.rings.corrected),
                        static_cast<unsigned long long>(r.rings.below_floor), static_cast<unsigned long long>(r.rings.above_limit),
                        static_cast<unsigned long long>(r.rings.not_finite), static_cast<double>(r.rings.max_abs));
        if(r.axis_search)
        {
            std::printf("axis search on: delta_s = %.4f px (the geometry file gave %.4f), candidate %u of %u at step %g, J_min / J_median = %.3g, "
                        "%u candidate(s) scored, %llu pair(s) skipped, %u frame(s) of %u row(s) from row %u in the pre-pass (%.3f s)\n",
                        static_cast<double>(r.axis.delta_s), static_cast<double>(r.axis_given), r.axis.best, r.axis_count, static_cast<double>(po.axis_step),
                        r.axis.cost_median > 0.0 ? r.axis.cost_min / r.axis.cost_median : 0.0, r.axis.scored,
                        static_cast<unsigned long long>(r.axis.skipped), r.axis_frames, po.axis_rows, r.axis.row_first, r.axis_prepass_s);
            if(r.axis.at_edge != 0u)
                std::printf("warning: the axis search's minimum has no scored neighbour on both sides or is not convex: delta_s is the best candidate itself; "
                            "widen the range of --find-axis\n");
            if(po.axis_only)
                return 0;
        }
        if(r.roll_search)
        {
            std::printf("roll search on: eta = %.4f deg, candidate %u of %u at step %g, J_min = %.6g, J_median = %.6g, J_min / J_median = %.3g, "
                        "%u candidate(s) scored, %llu pair(s) skipped, margins %u x %u, %u frame(s) in the pre-pass (%.3f s)\n",
                        static_cast<double>(r.roll.eta_deg), r.roll.best, r.roll_count, static_cast<double>(po.roll_step), r.roll.cost_min, r.roll.cost_median,
                        r.roll.cost_median > 0.0 ? r.roll.cost_min / r.roll.cost_median : 0.0, r.roll.scored,
                        static_cast<unsigned long long>(r.roll.skipped), r.roll.margin_x, r.roll.margin_y, r.roll_frames, r.roll_prepass_s);
            if(r.roll.at_edge != 0u)
                std::printf("warning: the roll search's minimum has no scored neighbour on both sides or is not convex: eta is the best candidate itself; "
                            "widen the range of --find-roll\n");
            if(po.roll_only)
                return 0;
        }
        if(r.detector_roll)
            std::printf("detector roll on: %.9g deg\n", static_cast<double>(r.roll_deg));
        if(r.starvation)
        {
            const auto& s = r.starvation_setting;
            const auto& c = r.starvation_counts;
            std::printf("starvation filter on: p0 %.9g, gain %.9g, radius %u, %llu pixel(s) filtered of %llu in %llu frame(s) (%.4g %%), %.4g %% of them "
                        "at the last level, whole frames (planned as --no-row-band)\n", static_cast<double>(s.p0), static_cast<double>(s.gain), s.radius,
                        static_cast<unsigned long long>(c.filtered), static_cast<unsigned long long>(r.starvation_pixels),
                        static_cast<unsigned long long>(c.frames),
                        r.starvation_pixels != 0u ? 100.0 * static_cast<double>(c.filtered) / static_cast<double>(r.starvation_pixels) : 0.0,
                        c.filtered != 0u ? 100.0 * static_cast<double>(c.last_level) / static_cast<double>(c.filtered) : 0.0);
        }
        if(r.scatter)
        {
            const auto& s = r.scatter_setting;
            const double l_x = static_cast<double>(r.scatter_l_x), l_y = static_cast<double>(r.scatter_l_y);
            std::printf("scatter correction on: A %.9g, alpha %.9g, beta %.9g, sigma %.9g and %.9g mm (%.4g x %.4g and %.4g x %.4g px), weight %.9g, "
                        "limit %.9g, %u iteration(s), margin %u, padded %u x %u, %u launch(es) per round, %llu scratch byte(s) per device, whole frames "
                        "(planned as --no-row-band)\n", static_cast<double>(s.amplitude), static_cast<double>(s.alpha), static_cast<double>(s.beta),
                        static_cast<double>(s.sigma1_mm), static_cast<double>(s.sigma2_mm), static_cast<double>(s.sigma1_mm) / l_x,
                        static_cast<double>(s.sigma1_mm) / l_y, static_cast<double>(s.sigma2_mm) / l_x, static_cast<double>(s.sigma2_mm) / l_y,
                        static_cast<double>(s.weight2), static_cast<double>(s.limit), s.iterations, s.margin, r.scatter_nx, r.scatter_ny,
                        2u * s.iterations + 1u, static_cast<unsigned long long>(r.scatter_scratch));
        }
        if(r.phase)
        {
            const double length = std::sqrt(static_cast<double>(r.phase_setting.alpha_mm2)) / (2.0 * 3.14159265358979323846);
            std::printf("phase retrieval on: alpha %.9g mm^2, kernel length %.4g x %.4g px, margin %u, floor %.9g, padded %u x %u, %llu scratch byte(s) per "
                        "device, whole frames (planned as --no-row-band)\n", static_cast<double>(r.phase_setting.alpha_mm2),
                        length / static_cast<double>(r.phase_l_x), length / static_cast<double>(r.phase_l_y), r.phase_setting.margin,
                        static_cast<double>(r.phase_setting.t_min), r.phase_nx, r.phase_ny, static_cast<unsigned long long>(r.phase_scratch));
        }
        if(r.beam_hardening)
        {
            if(r.bh_fitted)
                std::printf("beam-hardening fit on: degree %u, %u frame(s) into slices %u .. %u in the pre-pass (%.3f s), threshold %.9g, %llu object and "
                            "%llu air voxel(s), %llu not finite, level %.9g, residual %.6g before and %.6g after\n", r.bh.degree, r.bh_frames, r.bh_slice_first,
                            r.bh_slice_first + r.bh_slices - 1u, r.bh_prepass_s, static_cast<double>(r.bh_threshold),
                            static_cast<unsigned long long>(r.bh_counts.n_object), static_cast<unsigned long long>(r.bh_counts.n_air),
                            static_cast<unsigned long long>(r.bh_counts.n_not_finite), r.bh_fit.level, r.bh_fit.residual_before, r.bh_fit.residual_after);
            std::printf("beam hardening on: coefficients");
            for(std::uint32_t k = 0; k < r.bh.degree; ++k)
                std::printf("%s%.9g", k == 0u ? " " : ":", static_cast<double>(r.bh.c[k]));
            std::printf("\n");
        }
        if(r.denoise)
            std::printf("denoising on: 3-D bilateral filter, sigma_r %.9g, sigma_s %.9g voxel(s), radius %u (%u taps), %u halo slice(s) per slab side\n",
                        static_cast<double>(r.denoise_setting.sigma_r), static_cast<double>(r.denoise_setting.sigma_s), r.denoise_setting.radius,
                        (2u * r.denoise_setting.radius + 1u) * (2u * r.denoise_setting.radius + 1u) * (2u * r.denoise_setting.radius + 1u),
                        r.denoise_setting.radius);
        if(r.metal)
            std::printf("metal reduction on: %llu voxel(s) above %.9g collected, grow %u, min_path %.9g mm, %llu trace pixel(s) over all views, "
                        "%u frame(s) in the pre-pass (%.3f s), %llu pixel(s) replaced in %llu run(s) and %llu row(s) left in the main pass\n",
                        static_cast<unsigned long long>(r.metal_voxels), static_cast<double>(r.metal_threshold), r.metal_grow,
                        static_cast<double>(r.metal_min_path), static_cast<unsigned long long>(r.metal_trace_pixels), r.metal_frames, r.metal_prepass_s,
                        static_cast<unsigned long long>(r.metal_counts.replaced), static_cast<unsigned long long>(r.metal_counts.runs),
                        static_cast<unsigned long long>(r.metal_counts.rows_left));
        if(r.voxel_type != 0)
            std::printf("%llu voxel(s) written as %s over [%.9g, %.9g]: %llu below, %llu above, %llu not finite\n",
                        static_cast<unsigned long long>(r.voxels.voxels), r.voxel_type == PARIS_HIP_VOXEL_U8 ? "u8" : "u16", static_cast<double>(r.voxel_lo),
                        static_cast<double>(r.voxel_hi), static_cast<unsigned long long>(r.voxels.below), static_cast<unsigned long long>(r.voxels.above),
                        static_cast<unsigned long long>(r.voxels.not_finite));
        std::printf("volume %u x %u x %u (%d slab%s) -> %s in %.3f s\n", r.roi_geo.dim_x, r.roi_geo.dim_y, r.roi_geo.dim_z, r.info.num,
                    r.info.num == 1 ? "" : "s", r.output_file.c_str(), r.wall_s);
        if(r.devices.size() > 1 && r.shared_source)
            std::printf("shared frame source: %llu frames read from the files for %llu frame requests of the device threads\n",
                        static_cast<unsigned long long>(r.frames_read), static_cast<unsigned long long>(r.frames_requested));
        else if(r.devices.size() > 1)
            std::printf("frame source: one stream per device thread, each reads its slab's detector rows (%.2f detectors' worth per pass)\n",
                        r.rows_per_pass);
        for(const auto& s : r.skipped)
            std::printf("  skipped invalid file %s\n", s.c_str());
        for(const auto& d : r.devices)
        {
            std::printf("device %d: %u task(s), %u projections, %.0f detector rows per projection; host: setup %.3f s, source %.3f s%s, enqueue %.3f s, "
                        "waiting for the drain thread %.3f s (%s; drain thread: D2H %.3f s, save %.3f s)\n", d.device, d.tasks, d.projections,
                        d.tasks ? static_cast<double>(d.band_rows) / d.tasks : 0.0, d.setup_s, d.source_s,
                        po.read_ahead ? (" on the feed thread (the device thread waited " + std::to_string(d.source_wait_s).substr(0, 5) + " s for it)").c_str() : "",
                        d.enqueue_s, d.drain_wait_s, d.two_volumes ? "two volume buffers" : "one volume buffer", d.drain_s, d.save_s);
            for(const auto& s : d.skipped)
                std::printf("  skipped invalid file %s\n", s.c_str());
            std::printf("  H2D of device %d: %llu bytes of projection rows, as stored\n", d.device, static_cast<unsigned long long>(d.h2d_bytes));
        }
        return 0;
    }
    catch(const paris::stage_construction_error& e)
    {
        std::fprintf(stderr, "main(): Pipeline construction failed: %s\nAborting.\n", e.what());
        return 1;
    }
    catch(const paris::stage_runtime_error& e)
    {
        std::fprintf(stderr, "main(): Pipeline execution failed: %s\nAborting.\n", e.what());
        return 1;
    }
    catch(const std::exception& e)
    {
        std::fprintf(stderr, "main(): %s\nAborting.\n", e.what());
        return 1;
    }
}

// The calls of the C++ mirror that no projection loop reaches, one sub-command each, on raw arrays named on the command line
// (tests/test_gpu_cpp_mirror_stages.py compares what is written with the Python Backend's results, bit for bit).
//
// usage: paris_hip_mirror_calls bh <dim_x> <dim_y> <dim_z> <thr> <margin> <degree> <f_1.raw> ... <f_degree.raw> <hist.raw> <h_lo> <h_hi> <out>
//   f_k.raw: the basis volumes, dim_x x dim_y x dim_z float32 each; f_1 is the volume that is classified. hist.raw: uint64 bins of a
//   linear histogram over [h_lo, h_hi].
//   bh_classify(f_1, thr, margin)          -> <out>.labels     one byte per voxel
//   bh_gram(f_1 ... f_degree, the labels)  -> <out>.gram       (degree + 1)(degree + 2) / 2 doubles
//                                             <out>.counts     n_object, n_air, n_ignored, n_not_finite as uint64
//   bh_solve(the sums, the counts)         -> <out>.fit        the degree as one double, PARIS_HIP_BH_DEGREE_MAX coefficients as doubles
//                                                              (each float widens exactly), level, residual_before, residual_after
//   bh_threshold_from_histogram(hist)      -> <out>.threshold  one float32
//
// usage: paris_hip_mirror_calls frames <n_row> <n_col> <l_px_row> <l_px_col> <gap_rows> <in.raw> <out.raw>
//                                      scatter <A> <alpha> <beta> <sigma1> <sigma2> <w2> <limit> <iterations> <margin>
//                                    | phase <mm2> <t_min> <margin>
//   in.raw: 3 x (n_col + gap_rows) rows of n_row float32 -- three frames, each followed by gap_rows rows that belong to none. They
//   go into one pitched device buffer, so the frames are pitch * (n_col + gap_rows) bytes apart; set_scatter_correction() and
//   scatter_correction(), or set_phase_retrieval() and phase_retrieval(), with that stride and n_frames = 2; the buffer, all of it,
//   is written to out.raw: the third frame and the gaps must come back as they went in.
//
// usage: paris_hip_mirror_calls refused <n_row> <n_col> <l_px_row> <l_px_col> <delta_s> <delta_t> <d_so> <d_od> <delta_phi> <in.raw> <out.raw>
//   in one process: set_beam_hardening() with five coefficients, set_scatter_correction() with a limit of 1.5, set_phase_retrieval()
//   with a margin of 0 and set_metal_trace() with no view must each throw; then paris::weight() of the frame in in.raw (n_col rows of
//   n_row float32) must be the plain cosine weight, written to out.raw: a refused setting was not recorded for the thread.
//
// Exit status 0 and "ok" on success, 1 with the library's message where it refuses, 2 for a command line this program cannot read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "paris/stages.h"

namespace
{
    namespace be = paris::backend;

    template <typename T>
    auto read_raw(const std::string& path, std::size_t n) -> std::vector<T>
    {
        auto v = std::vector<T>(n);
        std::FILE* f = std::fopen(path.c_str(), "rb");
        const bool ok = f != nullptr && std::fread(v.data(), sizeof(T), n, f) == n && std::fgetc(f) == EOF;
        if(f != nullptr)
            std::fclose(f);
        if(!ok)
            throw paris::stage_runtime_error{"cannot read " + std::to_string(n) + " value(s) from " + path};
        return v;
    }

    template <typename T>
    void write_raw(const std::string& path, const T* p, std::size_t n)
    {
        std::FILE* f = std::fopen(path.c_str(), "wb");
        const bool ok = f != nullptr && std::fwrite(p, sizeof(T), n, f) == n;
        if(f != nullptr)
            std::fclose(f);
        if(!ok)
            throw paris::stage_runtime_error{"cannot write " + path};
    }

    auto u32(const char* s) -> std::uint32_t { return static_cast<std::uint32_t>(std::strtoul(s, nullptr, 10)); }
    auto f32(const char* s) -> float { return std::strtof(s, nullptr); }

    // a dense host array as a device volume of dim_x x dim_y x dim_z floats
    auto to_device(const float* src, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z) -> be::volume_device_type
    {
        auto h = be::make_volume_host(dim_x, dim_y, dim_z);
        std::memcpy(h.buf.get(), src, std::size_t{dim_x} * dim_y * dim_z * sizeof(float));
        auto d = be::make_volume_device(dim_x, dim_y, dim_z);
        be::copy_h2d(h, d);
        be::synchronize(); // h goes out of scope
        return d;
    }

    int bh(int argc, char** argv)
    {
        if(argc < 9)
            return 2;
        const auto dim_x = u32(argv[2]), dim_y = u32(argv[3]), dim_z = u32(argv[4]);
        const float thr = f32(argv[5]);
        const auto margin = u32(argv[6]), degree = u32(argv[7]);
        if(degree < 1u || degree > PARIS_HIP_BH_DEGREE_MAX || argc != static_cast<int>(8u + degree + 4u))
            return 2;
        const auto n = std::size_t{dim_x} * dim_y * dim_z;
        const auto out = std::string{argv[8 + degree + 3]};

        auto basis = std::vector<be::volume_device_type>{};
        auto d_f = std::vector<const float*>{};
        for(std::uint32_t k = 0; k < degree; ++k)
        {
            const auto f = read_raw<float>(argv[8 + k], n);
            basis.push_back(to_device(f.data(), dim_x, dim_y, dim_z));
            d_f.push_back(basis.back().buf.get());
        }
        // one byte per voxel, in a device allocation of whole floats
        const auto words = static_cast<std::uint32_t>((n + 3u) / 4u);
        auto d_labels = be::make_volume_device(words, 1u, 1u);
        auto* labels = reinterpret_cast<std::uint8_t*>(d_labels.buf.get());
        be::bh_classify(d_f[0], dim_x, dim_y, dim_z, thr, margin, labels);
        {
            auto h = be::make_volume_host(words, 1u, 1u);
            be::copy_d2h(d_labels, h);
            write_raw(out + ".labels", reinterpret_cast<const std::uint8_t*>(h.buf.get()), n);
        }
        auto gram = std::vector<double>((degree + 1u) * (degree + 2u) / 2u);
        const auto counts = be::bh_gram(d_f.data(), degree, labels, n, gram.data());
        write_raw(out + ".gram", gram.data(), gram.size());
        const std::uint64_t c[4] = {counts.n_object, counts.n_air, counts.n_ignored, counts.n_not_finite};
        write_raw(out + ".counts", c, 4u);
        const auto fit = be::bh_solve(gram.data(), degree, counts);
        double fitted[1 + PARIS_HIP_BH_DEGREE_MAX + 3] = {static_cast<double>(fit.setting.degree)};
        for(std::uint32_t k = 0; k < PARIS_HIP_BH_DEGREE_MAX; ++k)
            fitted[1u + k] = static_cast<double>(fit.setting.c[k]);
        fitted[1 + PARIS_HIP_BH_DEGREE_MAX] = fit.level;
        fitted[2 + PARIS_HIP_BH_DEGREE_MAX] = fit.residual_before;
        fitted[3 + PARIS_HIP_BH_DEGREE_MAX] = fit.residual_after;
        write_raw(out + ".fit", fitted, sizeof(fitted) / sizeof(fitted[0]));

        std::FILE* f = std::fopen(argv[8 + degree], "rb");
        if(f == nullptr)
            throw paris::stage_runtime_error{std::string{"cannot read "} + argv[8 + degree]};
        std::fseek(f, 0, SEEK_END);
        const auto n_bins = static_cast<std::size_t>(std::ftell(f)) / sizeof(std::uint64_t);
        std::fclose(f);
        const auto hist = read_raw<std::uint64_t>(argv[8 + degree], n_bins);
        const float otsu = be::bh_threshold_from_histogram(hist.data(), static_cast<std::uint32_t>(n_bins), f32(argv[8 + degree + 1]), f32(argv[8 + degree + 2]));
        write_raw(out + ".threshold", &otsu, 1u);
        return 0;
    }

    int frames(int argc, char** argv)
    {
        if(argc < 10)
            return 2;
        const auto n_row = u32(argv[2]), n_col = u32(argv[3]);
        const float l_px_row = f32(argv[4]), l_px_col = f32(argv[5]);
        const auto gap = u32(argv[6]);
        const auto what = std::string{argv[9]};
        const bool scatter = what == "scatter" && argc == 19, phase = what == "phase" && argc == 13;
        if(!scatter && !phase)
            return 2;
        const std::uint32_t n_frames = 3u, rows = n_frames * (n_col + gap);
        const auto in = read_raw<float>(argv[7], std::size_t{n_row} * rows);
        auto h = be::make_projection_host(n_row, rows);
        std::memcpy(h.buf.get(), in.data(), in.size() * sizeof(float));
        auto d = be::make_projection_device(n_row, rows);
        be::copy_h2d(h, d);
        const auto stride = d.buf.pitch() * (n_col + gap);
        if(scatter)
        {
            auto s = paris_hip_scatter_correction{};
            s.amplitude = f32(argv[10]);
            s.alpha = f32(argv[11]);
            s.beta = f32(argv[12]);
            s.sigma1_mm = f32(argv[13]);
            s.sigma2_mm = f32(argv[14]);
            s.weight2 = f32(argv[15]);
            s.limit = f32(argv[16]);
            s.iterations = u32(argv[17]);
            s.margin = u32(argv[18]);
            be::set_scatter_correction(s, n_row, n_col, l_px_row, l_px_col);
            be::scatter_correction(d.buf.get(), d.buf.pitch(), stride, n_frames - 1u, n_row, n_col);
            be::clear_scatter_correction();
        }
        else
        {
            be::set_phase_retrieval(f32(argv[10]), f32(argv[11]), u32(argv[12]), n_row, n_col, l_px_row, l_px_col);
            be::phase_retrieval(d.buf.get(), d.buf.pitch(), stride, n_frames - 1u, n_row, n_col);
            be::clear_phase_retrieval();
        }
        be::copy_d2h(d, h);
        write_raw(argv[8], h.buf.get(), in.size());
        return 0;
    }

    // true when the call threw stage_runtime_error, as a refused setter must
    template <typename F>
    bool refuses(F&& call)
    {
        try
        {
            call();
        }
        catch(const paris::stage_runtime_error&)
        {
            return true;
        }
        return false;
    }

    int refused(int argc, char** argv)
    {
        if(argc != 13)
            return 2;
        auto det = paris::detector_geometry{};
        det.n_row = u32(argv[2]);
        det.n_col = u32(argv[3]);
        det.l_px_row = f32(argv[4]);
        det.l_px_col = f32(argv[5]);
        det.delta_s = f32(argv[6]);
        det.delta_t = f32(argv[7]);
        det.d_so = f32(argv[8]);
        det.d_od = f32(argv[9]);
        det.delta_phi = f32(argv[10]);
        const auto in = read_raw<float>(argv[11], std::size_t{det.n_row} * det.n_col);
        const float c[5] = {1.f, 0.1f, 0.01f, 0.001f, 0.0001f};
        auto s = paris_hip_scatter_correction{0.05f, -0.15f, 1.f, 0.6f, 2.f, 0.5f, 1.5f, 4u, 10u}; // a limit of 1.5
        const std::uint64_t word = 0u;
        const bool all = refuses([&] { be::set_beam_hardening(c, 5u, det.n_row, det.n_col); })
                         && refuses([&] { be::set_scatter_correction(s, det.n_row, det.n_col, det.l_px_row, det.l_px_col); })
                         && refuses([&] { be::set_phase_retrieval(0.25f, 1e-5f, 0u, det.n_row, det.n_col, det.l_px_row, det.l_px_col); })
                         && refuses([&] { be::set_metal_trace(&word, 0u, det.n_row, det.n_col); });
        if(!all)
            throw paris::stage_runtime_error{"a setter took a setting the library refuses"};
        auto h = be::make_projection_host(det.n_row, det.n_col);
        std::memcpy(h.buf.get(), in.data(), in.size() * sizeof(float));
        auto d = paris::load(h);
        paris::weight(d, det); // a refused setting that was recorded for this thread would send the frame into a pass that has none
        be::copy_d2h(d, h);
        write_raw(argv[12], h.buf.get(), in.size());
        return 0;
    }
}

int main(int argc, char** argv)
{
    try
    {
        int rc = 2;
        if(argc >= 2 && !std::strcmp(argv[1], "bh"))
            rc = bh(argc, argv);
        else if(argc >= 2 && !std::strcmp(argv[1], "frames"))
            rc = frames(argc, argv);
        else if(argc >= 2 && !std::strcmp(argv[1], "refused"))
            rc = refused(argc, argv);
        if(rc == 2)
            std::fprintf(stderr, "usage: see the header of paris_hip_mirror_calls.cpp\n");
        else if(rc == 0)
            std::printf("ok\n");
        return rc;
    }
    catch(const paris::stage_construction_error& e)
    {
        std::fprintf(stderr, "construction failed: %s\n", e.what());
        return 1;
    }
    catch(const paris::stage_runtime_error& e)
    {
        std::fprintf(stderr, "execution failed: %s\n", e.what());
        return 1;
    }
}

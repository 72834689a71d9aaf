// C entry points over the host-only I/O code (HIS, DDBVF, directory listing, angle files) so that the CPU test suite
// can exercise it through ctypes. No GPU code in here; built as paris_amd/lib/libparis_io.so.
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "paris/ddbvf.h"
#include "paris/his.h"
#include "paris/source.h"

extern "C" {

// loads every frame of a HIS file; *data receives n_frames*dim_x*dim_y floats (free with paris_io_free).
// returns 0, or 1 when the file cannot be opened. A non-HIS file gives n_frames = 0.
int paris_io_his_load(const char* path, uint32_t* n_frames, uint32_t* dim_x, uint32_t* dim_y, float** data)
{
    try
    {
        const auto frames = paris::his::load(path);
        *n_frames = static_cast<uint32_t>(frames.size());
        *dim_x = frames.empty() ? 0 : frames[0].dim_x;
        *dim_y = frames.empty() ? 0 : frames[0].dim_y;
        *data = nullptr;
        if(!frames.empty())
        {
            const auto n = static_cast<size_t>(*dim_x) * *dim_y;
            *data = static_cast<float*>(std::malloc(n * frames.size() * sizeof(float)));
            for(size_t i = 0; i < frames.size(); ++i)
                std::memcpy(*data + n * i, frames[i].pixels.data(), n * sizeof(float));
        }
        return 0;
    }
    catch(const std::exception&) { return 1; }
}

void paris_io_free(void* p) { std::free(p); }

// his::mean_frame: the mean of all frames of a HIS file (dark / flat references); *data receives dim_x*dim_y floats (free with
// paris_io_free), NULL for a file without frames. Returns 0, or 1 when the file cannot be opened.
int paris_io_his_mean_frame(const char* path, uint32_t* n_frames, uint32_t* dim_x, uint32_t* dim_y, float** data)
{
    try
    {
        const auto m = paris::his::mean_frame(path);
        *n_frames = m.n_frames;
        *dim_x = m.dim_x;
        *dim_y = m.dim_y;
        *data = nullptr;
        if(m.n_frames != 0)
        {
            *data = static_cast<float*>(std::malloc(m.pixels.size() * sizeof(float)));
            std::memcpy(*data, m.pixels.data(), m.pixels.size() * sizeof(float));
        }
        return 0;
    }
    catch(const std::exception&) { return 1; }
}

int paris_io_his_save(const char* path, const float* frames, uint16_t n_frames, uint16_t dim_x, uint16_t dim_y, uint16_t number_type,
                      uint16_t image_header_size)
{
    try { paris::his::save(path, frames, n_frames, dim_x, dim_y, static_cast<paris::his::number_type>(number_type), image_header_size); return 0; }
    catch(const std::exception&) { return 1; }
}

// creates <path>.ddbvf and writes one slab; `create` != 0 truncates and writes the header first
int paris_io_ddbvf_write(const char* path, int create, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, const float* voxels,
                         uint32_t dim_z_slab, uint32_t first)
{
    try
    {
        paris::ddbvf::handle_type h;
        if(create)
            h = paris::ddbvf::create(path, dim_x, dim_y, dim_z);
        else
        {
            h.reset(new paris::ddbvf::handle);
            h->dim_x = dim_x; h->dim_y = dim_y; h->dim_z = dim_z; h->offset = 8;
            h->file = std::fopen((std::string{path} + ".ddbvf").c_str(), "r+b");
            if(!h->file)
                return 1;
        }
        paris::ddbvf::write(h, voxels, dim_x, dim_y, dim_z_slab, first);
        return 0;
    }
    catch(const std::runtime_error&) { return 2; }
    catch(const std::exception&) { return 1; }
}

// angle file -> malloc'd float array
int paris_io_read_angles(const char* path, uint32_t* n, float** out)
{
    try
    {
        const auto a = paris::read_angles(path);
        *n = static_cast<uint32_t>(a.size());
        *out = static_cast<float*>(std::malloc((a.size() + 1) * sizeof(float)));
        std::memcpy(*out, a.data(), a.size() * sizeof(float));
        return 0;
    }
    catch(const std::exception&) { return 1; }
}

// drains a source; returns per-frame idx / phi and the number of skipped files. idx_out/phi_out hold up to cap entries.
int paris_io_source_scan(const char* dir, int enable_angles, const char* angle_file, uint16_t quality, uint32_t cap, uint32_t* n_frames,
                         uint32_t* idx_out, float* phi_out, float* first_pixel_out, uint32_t* n_skipped)
{
    try
    {
        paris::source src{dir, enable_angles != 0, angle_file ? angle_file : "", quality};
        uint32_t n = 0;
        while(!src.drained())
        {
            const auto p = src.load_next();
            if(!p.valid())
                break;
            if(n < cap)
            {
                idx_out[n] = p.idx;
                phi_out[n] = p.phi;
                first_pixel_out[n] = p.pixels.empty() ? 0.f : p.pixels[0];
            }
            ++n;
        }
        *n_frames = n;
        *n_skipped = static_cast<uint32_t>(src.skipped_files().size());
        return 0;
    }
    catch(const std::exception&) { return 1; }
}
// the same scan through frame_stream: frame i is written into data + i * dim_x * dim_y * size (caller-filled with a sentinel),
// only rows [row_first, row_first + row_count); size = 4 (floats), raw: the frame's pixels as stored, at most 4 bytes each, their
// type (his::pixel_type) in type_out. Frames of another size end the scan with return code 3.
static int stream_scan(bool raw, const char* dir, int enable_angles, const char* angle_file, uint16_t quality, uint32_t dim_x, uint32_t dim_y,
                       uint32_t row_first, uint32_t row_count, uint32_t cap, uint32_t* n_frames, uint32_t* idx_out, float* phi_out,
                       void* data, int32_t* type_out, uint32_t* n_skipped)
{
    try
    {
        paris::frame_stream src{dir, enable_angles != 0, angle_file ? angle_file : "", quality};
        const auto frame = static_cast<size_t>(dim_x) * dim_y * sizeof(float);
        auto scratch = std::vector<uint8_t>(frame);
        uint32_t n = 0;
        for(;;)
        {
            void* dst = n < cap ? static_cast<uint8_t*>(data) + static_cast<size_t>(n) * frame : scratch.data();
            const auto info = raw ? src.next_raw(dst, dim_x, dim_y, row_first, row_count)
                                  : src.next(static_cast<float*>(dst), dim_x, dim_y, row_first, row_count);
            if(!info.valid())
                break;
            if(info.dim_x != dim_x || info.dim_y != dim_y)
                return 3;
            if(n < cap)
            {
                idx_out[n] = info.idx;
                phi_out[n] = info.phi;
                if(type_out)
                    type_out[n] = info.pixel;
            }
            ++n;
        }
        *n_frames = n;
        *n_skipped = static_cast<uint32_t>(src.skipped_files().size());
        return 0;
    }
    catch(const std::exception&) { return 1; }
}

int paris_io_stream_scan(const char* dir, int enable_angles, const char* angle_file, uint16_t quality, uint32_t dim_x, uint32_t dim_y,
                         uint32_t row_first, uint32_t row_count, uint32_t cap, uint32_t* n_frames, uint32_t* idx_out, float* phi_out,
                         float* data, uint32_t* n_skipped)
{
    return stream_scan(false, dir, enable_angles, angle_file, quality, dim_x, dim_y, row_first, row_count, cap, n_frames, idx_out, phi_out,
                       data, nullptr, n_skipped);
}

int paris_io_stream_scan_raw(const char* dir, int enable_angles, const char* angle_file, uint16_t quality, uint32_t dim_x, uint32_t dim_y,
                             uint32_t row_first, uint32_t row_count, uint32_t cap, uint32_t* n_frames, uint32_t* idx_out, float* phi_out,
                             void* data, int32_t* type_out, uint32_t* n_skipped)
{
    return stream_scan(true, dir, enable_angles, angle_file, quality, dim_x, dim_y, row_first, row_count, cap, n_frames, idx_out, phi_out,
                       data, type_out, n_skipped);
}

// shared_frames under `n_threads` consumers: thread i reads rows [row_first[i], row_first[i] + row_count[i]) of every frame into
// data + (i * cap + n) * dim_x * dim_y * 4 bytes (caller-filled with a sentinel): floats, or raw: the pixels as stored, their type in
// type_out[i * cap + n]; thread i sleeps delay_us[i] microseconds per frame, so a slow consumer falls out of the ring (capacity) and
// takes its own fallback stream. counters: produced, served, reread.
static int shared_scan(bool raw, const char* dir, int enable_angles, const char* angle_file, uint16_t quality, uint32_t dim_x, uint32_t dim_y,
                       uint32_t n_threads, const uint32_t* row_first, const uint32_t* row_count, const uint32_t* delay_us, uint32_t capacity,
                       uint32_t cap, uint32_t* n_frames, uint32_t* idx_out, float* phi_out, void* data, int32_t* type_out, uint64_t* counters)
{
    try
    {
        paris::shared_frames shared{dir, enable_angles != 0, angle_file ? angle_file : "", quality, dim_x, dim_y, capacity};
        auto failed = std::vector<int>(n_threads, 0);
        auto workers = std::vector<std::thread>{};
        const auto frame = static_cast<size_t>(dim_x) * dim_y * sizeof(float);
        for(uint32_t i = 0; i < n_threads; ++i)
            workers.emplace_back([&, i] {
                try
                {
                    auto cur = paris::shared_frames::cursor{};
                    auto scratch = std::vector<uint8_t>(frame);
                    uint32_t n = 0;
                    for(;;)
                    {
                        void* dst = n < cap ? static_cast<uint8_t*>(data) + (static_cast<size_t>(i) * cap + n) * frame : scratch.data();
                        const auto info = raw ? shared.next_raw(cur, dst, dim_x, dim_y, row_first[i], row_count[i])
                                              : shared.next(cur, static_cast<float*>(dst), dim_x, dim_y, row_first[i], row_count[i]);
                        if(!info.valid())
                            break;
                        if(n < cap)
                        {
                            idx_out[static_cast<size_t>(i) * cap + n] = info.idx;
                            phi_out[static_cast<size_t>(i) * cap + n] = info.phi;
                            if(type_out)
                                type_out[static_cast<size_t>(i) * cap + n] = info.pixel;
                        }
                        ++n;
                        if(delay_us[i])
                            std::this_thread::sleep_for(std::chrono::microseconds(delay_us[i]));
                    }
                    n_frames[i] = n;
                }
                catch(const std::exception&) { failed[i] = 1; }
            });
        for(auto& w : workers)
            w.join();
        for(int f : failed)
            if(f)
                return 1;
        const auto st = shared.stats();
        counters[0] = st.produced;
        counters[1] = st.served;
        counters[2] = st.reread;
        return 0;
    }
    catch(const std::exception&) { return 1; }
}

int paris_io_shared_scan(const char* dir, int enable_angles, const char* angle_file, uint16_t quality, uint32_t dim_x, uint32_t dim_y,
                         uint32_t n_threads, const uint32_t* row_first, const uint32_t* row_count, const uint32_t* delay_us, uint32_t capacity,
                         uint32_t cap, uint32_t* n_frames, uint32_t* idx_out, float* phi_out, float* data, uint64_t* counters)
{
    return shared_scan(false, dir, enable_angles, angle_file, quality, dim_x, dim_y, n_threads, row_first, row_count, delay_us, capacity, cap,
                       n_frames, idx_out, phi_out, data, nullptr, counters);
}

int paris_io_shared_scan_raw(const char* dir, int enable_angles, const char* angle_file, uint16_t quality, uint32_t dim_x, uint32_t dim_y,
                             uint32_t n_threads, const uint32_t* row_first, const uint32_t* row_count, const uint32_t* delay_us, uint32_t capacity,
                             uint32_t cap, uint32_t* n_frames, uint32_t* idx_out, float* phi_out, void* data, int32_t* type_out, uint64_t* counters)
{
    return shared_scan(true, dir, enable_angles, angle_file, quality, dim_x, dim_y, n_threads, row_first, row_count, delay_us, capacity, cap,
                       n_frames, idx_out, phi_out, data, type_out, counters);
}
}

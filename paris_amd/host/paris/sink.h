// Volume sink: one DDBVF file that every device thread writes its slabs into (src/sink.cpp:39-94) -- or, for voxels quantised to 8 or
// 16 bits, one .raw file with a MetaImage header beside it (mhd.h).
// Repair of quirk Q4: the slab's first slice is passed explicitly (the reference writes every slab at volume::off,
// which nothing ever sets, so all slabs land on slice 0).
#ifndef PARIS_AMD_HOST_SINK_H_
#define PARIS_AMD_HOST_SINK_H_

#include <mutex>
#include <string>

#include <sys/stat.h>

#include "ddbvf.h"
#include "mhd.h"
#include "types.h"

namespace paris
{
    // src/filesystem.cpp:69-90 (mkdir -p)
    inline auto create_directory(const std::string& path) -> bool
    {
        struct stat st{};
        if(::stat(path.c_str(), &st) == 0)
        {
            if(S_ISDIR(st.st_mode))
                return true;
            throw std::runtime_error{path + " exists but is not a directory."};
        }
        for(std::size_t pos = 1; pos <= path.size(); ++pos)
            if(pos == path.size() || path[pos] == '/')
            {
                const auto sub = path.substr(0, pos);
                if(::mkdir(sub.c_str(), 0777) != 0 && errno != EEXIST)
                    return false;
            }
        return true;
    }

    class sink
    {
    public:
        // voxel_bytes 0: float voxels into a DDBVF file. 1 or 2: quantised voxels into `prefix`.raw; `prefix`.mhd is written by
        // set_window(), which the caller calls at once when it knows the window and the drain thread calls when it has chosen one.
        sink(const std::string& path, const std::string& prefix, const volume_geometry& vol_geo, std::uint32_t voxel_bytes = 0u)
        : path_{path}, prefix_{prefix}, vol_geo_(vol_geo), voxel_bytes_{voxel_bytes}
        {
            try
            {
                if(path_.empty() || path_.back() != '/')
                    path_ += '/';
                path_ += prefix;
                if(!create_directory(path))
                    throw stage_construction_error{"sink::sink() failed to create output directory at " + path};
                if(voxel_bytes_ == 0u)
                    handle_ = ddbvf::create(path_, vol_geo_.dim_x, vol_geo_.dim_y, vol_geo_.dim_z);
                else
                    raw_ = mhd::create(path_, vol_geo_.dim_x, vol_geo_.dim_y, vol_geo_.dim_z, voxel_bytes_);
            }
            catch(const std::system_error& se) { throw stage_runtime_error{std::string{"sink::sink() failed: "} + se.what()}; }
            catch(const std::runtime_error& re) { throw stage_construction_error{std::string{"sink::sink() failed: "} + re.what()}; }
        }

        auto file_path() const -> std::string { return path_ + (voxel_bytes_ == 0u ? ".ddbvf" : ".mhd"); }

        // the grey window of a quantised volume: writes the MetaImage header, which records it
        auto set_window(float lo, float hi) -> void
        {
            try
            {
                mhd::write_header(path_, prefix_ + ".raw", *raw_, vol_geo_.l_vx_x, vol_geo_.l_vx_y, vol_geo_.l_vx_z, lo, hi,
                                  voxel_bytes_ == 1u ? 255u : 65535u);
            }
            catch(const std::exception& e) { throw stage_runtime_error{std::string{"sink::set_window() failed: "} + e.what()}; }
            std::lock_guard<std::mutex> lock{window_m_};
            window_lo_ = lo;
            window_hi_ = hi;
        }
        auto window(float& lo, float& hi) -> void
        {
            std::lock_guard<std::mutex> lock{window_m_};
            lo = window_lo_;
            hi = window_hi_;
        }

        // host voxels of one slab (or a chunk of it) starting at global slice `first`. The reference serialises this with a
        // static mutex (src/sink.cpp:79-81) because its writer moves a shared stream position; ddbvf::write uses positioned
        // writes, so device threads write their disjoint slice ranges concurrently.
        auto save(const float* voxels, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z, std::uint32_t first) -> void
        {
            try { ddbvf::write(handle_, voxels, dim_x, dim_y, dim_z, first); }
            catch(const std::system_error& se) { throw stage_runtime_error{std::string{"sink::save() failed: "} + se.what()}; }
            catch(const std::runtime_error& re) { throw stage_runtime_error{std::string{"sink::save() failed: "} + re.what()}; }
        }

        // the same for quantised voxels, 1 or 2 bytes each
        auto save_quantised(const void* voxels, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z, std::uint32_t first) -> void
        {
            try { mhd::write(raw_, voxels, dim_x, dim_y, dim_z, first); }
            catch(const std::system_error& se) { throw stage_runtime_error{std::string{"sink::save() failed: "} + se.what()}; }
            catch(const std::runtime_error& re) { throw stage_runtime_error{std::string{"sink::save() failed: "} + re.what()}; }
        }

    private:
        std::string path_, prefix_;
        ddbvf::handle_type handle_;
        mhd::handle_type raw_;
        volume_geometry vol_geo_;
        std::uint32_t voxel_bytes_ = 0;
        std::mutex window_m_;
        float window_lo_ = 0.f, window_hi_ = 0.f;
    };
}

#endif

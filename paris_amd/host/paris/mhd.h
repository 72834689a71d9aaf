// MetaImage volume files for 8- and 16-bit voxels: `path`.raw holds the voxels, x fastest, no header,
// slice `first` at dim_x * dim_y * first * bytes-per-voxel; `path`.mhd is the text header that names it. The two intensity keys
// record the grey window: value = Slope * stored + Offset.
#ifndef PARIS_AMD_HOST_MHD_H_
#define PARIS_AMD_HOST_MHD_H_

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <system_error>

#include "ddbvf.h"

namespace paris
{
    namespace mhd
    {
        struct handle
        {
            std::uint32_t dim_x = 0, dim_y = 0, dim_z = 0, voxel_bytes = 0;
            std::FILE* file = nullptr;
            ~handle() { if(file) std::fclose(file); }
        };
        using handle_type = std::unique_ptr<handle>;

        // creates `path`.raw, empty; voxel_bytes is 1 or 2
        inline auto create(const std::string& path, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z, std::uint32_t voxel_bytes)
            -> handle_type
        {
            auto h = handle_type{new handle};
            h->dim_x = dim_x;
            h->dim_y = dim_y;
            h->dim_z = dim_z;
            h->voxel_bytes = voxel_bytes;
            const auto full = path + ".raw";
            h->file = std::fopen(full.c_str(), "w+b");
            if(!h->file)
                throw std::system_error{errno, std::generic_category(), "mhd::create(): " + full};
            return h;
        }

        // writes `path`.mhd for the voxels of `h`; data_file is the .raw's name as the header refers to it (no directory). lo and hi
        // are the window's ends, levels the largest stored value (255 or 65535).
        inline void write_header(const std::string& path, const std::string& data_file, const handle& h, float l_vx_x, float l_vx_y,
                                 float l_vx_z, float lo, float hi, std::uint32_t levels)
        {
            const auto full = path + ".mhd";
            auto* f = std::fopen(full.c_str(), "w");
            if(!f)
                throw std::system_error{errno, std::generic_category(), "mhd::write_header(): " + full};
            const double slope = (static_cast<double>(hi) - static_cast<double>(lo)) / static_cast<double>(levels);
            const int ok = std::fprintf(f,
                                        "ObjectType = Image\nNDims = 3\nDimSize = %u %u %u\nElementSpacing = %.9g %.9g %.9g\nElementType = %s\n"
                                        "BinaryData = True\nBinaryDataByteOrderMSB = False\nElementToIntensityFunctionSlope = %.9g\n"
                                        "ElementToIntensityFunctionOffset = %.9g\nElementDataFile = %s\n",
                                        h.dim_x, h.dim_y, h.dim_z, static_cast<double>(l_vx_x), static_cast<double>(l_vx_y), static_cast<double>(l_vx_z),
                                        h.voxel_bytes == 1u ? "MET_UCHAR" : "MET_USHORT", slope, static_cast<double>(lo), data_file.c_str());
            const int closed = std::fclose(f);
            if(ok < 0 || closed != 0)
                throw std::runtime_error{"mhd::write_header(): cannot write " + full};
        }

        // writes a slab of dim_z_slab slices starting at global slice `first`, with ddbvf::write's positioned writes: slabs of different
        // device threads can be written concurrently
        inline void write(handle_type& h, const void* voxels, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z_slab, std::uint32_t first)
        {
            if(!h || voxels == nullptr)
                return;
            if(first >= h->dim_z)
                throw std::runtime_error{"mhd::write(): Starting position out of bounds"};
            if(dim_x != h->dim_x || dim_y != h->dim_y || dim_z_slab > h->dim_z - first)
                throw std::runtime_error{"mhd::write(): Attempting to save volume to file with wrong dimensions"};
            const auto slice = static_cast<std::uint64_t>(dim_x) * dim_y * h->voxel_bytes;
            ddbvf::write_at(fileno(h->file), voxels, slice * dim_z_slab, slice * first, "mhd::write()");
        }
    }
}

#endif

// The repair plan of a detector defect map: host data only, built by defect_plan.cpp -- the one place the
// rule of include/paris_hip.h is implemented -- and copied to the device as it is by defect_map.hip.
#ifndef PARIS_HIP_DEFECT_PLAN_H_
#define PARIS_HIP_DEFECT_PLAN_H_

#include <cstdint>
#include <vector>

#include "paris_hip.h"

struct paris_hip_defect_plan
{
    uint32_t dim_x = 0, dim_y = 0;
    paris_hip_defect_stats stats{};
    // CSR over the repairable defects, sorted row-major: defect k is pixel defect[k] (y * dim_x + x) and sums the pixels
    // source[first_source[k] .. first_source[k + 1]) with the weights at the same positions
    std::vector<uint32_t> defect, first_source, source;
    std::vector<float> weight;
    std::vector<uint32_t> row_start; // dim_y + 1: the defects of row y are defect[row_start[y] .. row_start[y + 1])
};

#endif

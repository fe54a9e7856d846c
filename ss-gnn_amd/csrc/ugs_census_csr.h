// ugs_census_csr.h -- what ugs_census_csr.hip (kernels) and ugs_census_csr.cpp (the entries ugs_graphlet_census_csr and
// ugs_graphlet_vertex_census_csr of include/ugs_mi355.h, which states the law) share.  DESIGN.md section 19.5.
#pragma once
#include "ugs_device.h"

// The call: the batch as a simple CSR on the device.  rowptr [N + 1] and col [M] hold every vertex's neighbours, global ids, strictly
// ascending, symmetric, inside the vertex's own graph; ugs_census_csr_validate says whether they do.
struct UgsCsrCall {
    const int64_t *ptr;                      // [G + 1]
    const int64_t *rowptr;                   // [N + 1]
    const int32_t *col;                      // [M]
    int64_t G, N, M;
    int k;
    unsigned long long budget;               // limit: a graph with more sets fails
    unsigned long long *gcount;              // [G] the graphs' set counts, zeroed by the entry; exact for a graph within the budget
    int32_t *flag;                           // validation: set to 1 if ptr, rowptr or col break a precondition
};

// One launch: *flag = 1 unless ptr is non-decreasing from ptr[0] >= 0 to ptr[G] = N, rowptr is non-decreasing from 0 to M, and every
// entry lies in its row's graph, differs from its row's vertex, exceeds its predecessor in the row and has its mirror.  Reads nothing
// outside ptr [G + 1], rowptr [N + 1] and col [M], whatever they hold.
hipError_t ugs_census_csr_validate(const UgsCsrCall &c, hipStream_t s);
// The search over a validated CSR, k = 1 ... 7; z.counts / z.gdv are zeroed by the entry.  UgsCensus::keys is not read.
hipError_t ugs_census_csr_census(const UgsCsrCall &c, const UgsCensus &z, hipStream_t s);
hipError_t ugs_census_csr_vertex(const UgsCsrCall &c, const UgsVertexCensus &z, hipStream_t s);
// Behind the search: zeros for every graph whose gcount is past the budget.  The entry reads gcount back for the status anyway and
// launches these only in a call where some graph failed.
hipError_t ugs_census_csr_census_clear(const UgsCsrCall &c, const UgsCensus &z, hipStream_t s);
hipError_t ugs_census_csr_vertex_clear(const UgsCsrCall &c, const UgsVertexCensus &z, hipStream_t s);

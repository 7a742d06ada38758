// The two-build convention.  The compressible and the advection units are compiled twice from one
// source (build.py, UNITS): PYRO_FAST=0 with -ffp-contract=off, the bit-faithful build, whose host
// functions live in pyro::exact, and PYRO_FAST=1 with -ffp-contract=fast, the contracted build, in
// pyro::fastm.  A unit opens `namespace pyro { namespace PYRO_NS {`; whoever calls across the seam
// picks the build with PYRO_BUILD.  (swe.hip keeps a pair of namespaces of its own.)
#pragma once

#ifndef PYRO_FAST
#define PYRO_FAST 0
#endif
#if PYRO_FAST
#define PYRO_NS fastm
#else
#define PYRO_NS exact
#endif

// `call` in the build that `fast` names: the call text is written once, so the two builds cannot be
// handed different arguments
#define PYRO_BUILD(fast, call) ((fast) ? ::pyro::fastm::call : ::pyro::exact::call)

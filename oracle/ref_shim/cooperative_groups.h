// Forwarding header of the reference-kernel build (oracle/ref_build.py): the name the reference sources include, served by ROCm.
#pragma once
#include <hip/hip_cooperative_groups.h>

// Forwarding header of the reference-kernel build (oracle/ref_build.py): the name the reference sources include, served by ROCm.
#pragma once
// (nothing: the reference sources include this header and use no reduction from it)

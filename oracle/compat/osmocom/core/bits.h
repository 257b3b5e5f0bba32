/* Stand-in for libosmocore's <osmocom/core/bits.h>: the three bit typedefs, all that grgsm_vitac.cpp takes from it. */
#pragma once
#include <stdint.h>
typedef int8_t sbit_t;
typedef uint8_t ubit_t;
typedef uint8_t pbit_t;

// mssim_limits.h -- capacities of the control-step kernel (mssim_solve16.h) that the host has to know as well: what
// mssim_create checks a model against (mssim_model_pack.h) and sizes its allocations with. Plain macros, no HIP.
#pragma once

#define MAXC 52  // solver blocks per env: contact points + torsional blocks (overflow is reported, never silent); 4 envs x the LDS tables = 40.0 KB per block, 4 blocks per CU
#define S16_LANES 16
#define S16_MAX_FREE_(nr) ((nr) == 4 ? 6 : 2)  // free bodies per env: two per 16-lane row that holds free bodies
#define S16_MAX_KIN 6
#define S16_MAX_SHAPE_(nr) ((nr) == 4 ? 64 : ((nr) > 1 ? 48 : 28))  // shapes per model: a lane builds the world-table entries of two (NR > 1: all lanes of the env)
// candidate pairs per model: the cull stages the whole pair table in the [896] narrowphase scratch of an env (S16_NP_SCR
// in mssim_solve16.h), 56 rounds of 16 pairs
#define S16_MAX_PAIR (56 * 16)
#define S16_PCM_LEN 48            // floats per cache slot: pair npts stamp flags | relp(3) - | relR(9) n_loc(3) | 4 x (pA(3) pB(3) gap)

// Backbones built on the generic layer-graph engine (gnet.h): constructors only; every C-ABI entry point that takes a handle
// (ptta_api.hip, msgchn_step.hip, msgchn_head.hip) forwards to the GNet methods.
#pragma once
#include "gnet.h"

// legacy_offset: bit 0 legacy offsets, bit 1 the SyncBN-adapted list, bit 2 the 2layers block, bit 3 the meta-only adapted list; flags (CostDCNet): bit 0 SyncBN-adapted, bit 1 2layers
GNet* nlspn_create(int n, int h, int w, const ptta_hparams* hp, int legacy_offset, int* rc);         // nlspn_api.hip
GNet* costdc_create(int n, int h, int w, const ptta_hparams* hp, float max_depth, int flags, int* rc);          // costdc_api.hip

// rescorer_handle.h -- the object behind ppasr_rescorer (created in capi_rescore.hip; capi_attdecode.hip decodes with it)
#pragma once
#include "capi_internal.h"
#include "rescore_kernels.h"

struct ppasr_rescorer_s {
  ppasr_rescorer_desc desc;
  ppasr_model_s store;  // owns the device memory (the loader uploads through it)
  RescoreW W{};
};

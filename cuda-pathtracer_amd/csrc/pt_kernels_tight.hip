// pt_kernels_tight.hip — the tight copy of the restart kernel's flat deferring form (PT_RS_FLAT_SKIP_TIGHT; pt_device.h: kRestartForms,
// RestartTraits::tight), in a translation unit of its own.
//
// The form is one more pt_megakernel_restart<LDS_RESIDENT, VARIANT> and reads its row like every other.  Compiled beside the others it
// moved the compiler's register allocation and scheduling in four of them (the three deferring forms and the instrumented one),
// whose code is pinned byte for byte (tests/golden/kernel_isa_digests.json); a unit of its own cannot.  This unit compiles the SAME
// source with PT_TIGHT_BUILD: of its host half only the restart kernel's entry table, which here names the tight forms alone,
// in namespace ptamd_tight.  pt_kernels.hip asks ptamd_tight_restart_entry for the entry where its own table would instantiate one.
// The form's kernel body is its own: with PT_TIGHT_BUILD pt_kernels.hip includes pt_tight_body.h behind the template's body, an
// explicit specialisation for <true, PT_RS_FLAT_SKIP_TIGHT>, which the entry table then names; so is its shading half
// (pt_tight_shade.h, which restates path_post for the form's launches).  The camera, the light loop, the round (traverse_round_tight)
// and the pools are the shared source's.
#define PT_TIGHT_BUILD 1
#define ptamd ptamd_tight
#include "pt_kernels.hip"

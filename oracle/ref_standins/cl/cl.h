// oracle/ref_standins -- TEST INFRASTRUCTURE ONLY.  Stand-in for a platform/SDK header that the reference's template/precomp.h includes
// unconditionally; written for this project, it holds only what that header needs to parse (see oracle/Makefile, _ref/libref_hotpath.so).
#pragma once
// opaque handles: only pointers to them are ever declared
typedef struct agpt_standin_cl_mem* cl_mem;
typedef struct agpt_standin_cl_event* cl_event;
typedef struct agpt_standin_cl_kernel* cl_kernel;
typedef struct agpt_standin_cl_program* cl_program;
typedef struct agpt_standin_cl_command_queue* cl_command_queue;
typedef struct agpt_standin_cl_context* cl_context;
typedef struct agpt_standin_cl_device_id* cl_device_id;

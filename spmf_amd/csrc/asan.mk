# Host-side AddressSanitizer build of the C-ABI layer (api_*.hip: argument checks, workspace
# carving, descriptor handling, RCCL binding; layout.hip: geometry, buffer carving, the
# argument checks of the layout builder) linked against the regular kernel objects.
# CPU only -- tests/test_host.py loads it under LD_PRELOAD=$(ASAN_RT) and walks the error
# paths; GPU sanitizer runs are not available on the pool.
ASAN_RT ?= $(shell $(HIPCC) -print-file-name=libclang_rt.asan-x86_64.so 2>/dev/null)
ASAN_LIB = ../libspmf_hip_asan.so
%_asan.o: %.hip $(HDRS)
	$(HIPCC) $(CXXFLAGS) -O1 -g -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer -c $< -o $@
# instrumented: the files with host-side logic behind the C-ABI
HOST_SRCS = api_ctx.hip api_step.hip api_stream.hip api_points.hip api_graph.hip api_comm.hip api_vi.hip layout.hip
ASAN_OBJS = $(HOST_SRCS:.hip=_asan.o) $(filter-out $(HOST_SRCS:.hip=.o),$(OBJS))
$(ASAN_LIB): $(ASAN_OBJS) exports.map
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -fsanitize=address -shared-libsan -Wl,--version-script=exports.map $(ASAN_OBJS) -o $@ -ldl
asan: $(ASAN_LIB)
	@echo $(ASAN_RT)

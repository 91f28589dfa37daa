# Top-level build: HIP library (gfx950), host mirror library, CPU oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := shenqi_amd/csrc
LIBDIR := shenqi_amd/lib
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Iinclude
# longest compile first: make -j starts the jobs in this order, and the build is as long as its last job (fft3d.hip alone takes about as
# long as a quarter of all the others together)
HIPSRC := $(addprefix $(CSRC)/,$(addsuffix .hip,fft3d exchange fof tree_build sph_winds sph grav_walk heiii toptree dynamics sph_bh sph_ngbsums sph_capi capi uvbg grav_group lens zeldovich glass thermal timestep pm sph_resident yields cooling cooling_host sfr sfr_host domain snapshot lightcone startup stats nulra nulra_host))
HIPOBJ := $(patsubst $(CSRC)/%.hip,$(LIBDIR)/%.o,$(HIPSRC))

all: $(LIBDIR)/libshenqi_hip.so host oracle

$(LIBDIR)/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.hpp) include/shenqi_hip.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/libshenqi_hip.so: $(HIPOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(HIPOBJ) -L/opt/rocm/lib -lhipfft -Wl,-rpath,/opt/rocm/lib

host: $(LIBDIR)/libshenqi_hip.so
	$(MAKE) -C shenqi_amd/host

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(LIBDIR); $(MAKE) -C oracle clean; $(MAKE) -C shenqi_amd/host clean
.PHONY: all host oracle clean
